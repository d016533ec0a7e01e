"""CPU checks of the model-inputs entry points (wp_linear_encode_inputs / wp_get_inputs_stats): what they answer without
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


def test_empty_inputs_need_no_device():
    v = W.Vocab(VOCAB)
    out = v.encode_inputs(a=["", ""], b=["", ""], max_len=5, cls_id=101, sep_id=102, pad_id=7)
    assert sorted(out) == ["input_ids", "lengths", "sample", "token_type_ids"]
    assert all(x.dtype == np.int32 for x in out.values())
    assert out["input_ids"].tolist() == [[101, 102, 102, 7, 7]] * 2
    assert out["token_type_ids"].tolist() == [[0, 0, 1, 0, 0]] * 2
    assert out["lengths"].tolist() == [3, 3] and out["sample"].tolist() == [0, 1]
    out = v.encode_inputs(a=["", "", ""], max_len=4, cls_id=101, sep_id=102, pad_id=7, offsets="byte")
    assert out["input_ids"].tolist() == [[101, 102, 7, 7]] * 3 and out["token_type_ids"].tolist() == [[0] * 4] * 3
    assert out["lengths"].tolist() == [2] * 3 and out["sample"].tolist() == [0, 1, 2]
    assert out["offsets"].dtype == np.uint32 and out["offsets"].shape == (3, 4, 2) and not out["offsets"].any()
    out = v.encode_inputs(text=b"\n\n", doc_offsets=[0, 1, 2], pairs=True, max_len=3, sep_id=9)
    assert out["input_ids"].tolist() == [[9, 9, 0]] and out["token_type_ids"].tolist() == [[0, 1, 0]] and out["lengths"].tolist() == [2]
    out = v.encode_inputs(a=[""], b=[""], max_len=2, truncation="only_second", stride=1)  # no specials: B = 2, one empty window
    assert out["input_ids"].tolist() == [[0, 0]] and out["lengths"].tolist() == [0] and out["sample"].tolist() == [0]
    for kw in (dict(a=[]), dict(a=[], b=[]), dict(text=b""), dict(text=b"", pairs=True)):
        out = v.encode_inputs(max_len=6, cls_id=1, offsets="char", **kw)
        assert out["input_ids"].shape == (0, 6) and out["token_type_ids"].shape == (0, 6) and out["offsets"].shape == (0, 6, 2)
        assert out["lengths"].shape == (0,) and out["sample"].shape == (0,)


def test_argument_errors_come_before_the_device():
    v = W.Vocab(VOCAB)
    a, b = ["ab", "a"], ["b", ""]
    for kw, msg in ((dict(truncation="only_first", stride=-2), "stride"),
                    (dict(max_len=0), "max_len"), (dict(max_len=-1), "max_len"), (dict(max_len=2, cls_id=1, sep_id=2), "max_len"),
                    (dict(max_len=8, stride=0), "windows"), (dict(max_len=8, stride=3, truncation="longest_first"), "windows"),
                    (dict(max_len=8, cls_id=1, sep_id=2, truncation="only_first", stride=5), "no room for a window"),
                    (dict(max_len=3, cls_id=1, sep_id=2, truncation="only_second"), "no room for a window"),
                    (dict(max_len=8, offsets="word"), "unit")):
        for docs in (dict(a=a, b=b), dict(a=["", ""], b=["", ""])):  # (and for inputs that need no device)
            with pytest.raises(W.WordPieceError, match=msg):
                v.encode_inputs(**docs, **kw)
    with pytest.raises(W.WordPieceError, match="only_second needs pairs"):
        v.encode_inputs(a=a, max_len=8, truncation="only_second")
    with pytest.raises(W.WordPieceError, match="pairs must be 0 or 1"):
        v.encode_inputs(text=b"ab\na\n", pairs=2, max_len=8)
    with pytest.raises(W.WordPieceError, match="truncation"):
        v.encode_inputs(a=a, max_len=8, truncation="shortest_first")
    # the odd-row rule: explicit rows and the lines of a text, with and without the final newline
    for kw in (dict(text=b"ab\na\nb\n", doc_offsets=[0, 3, 5, 7]), dict(text=b"ab\na\nb\n"), dict(text=b"ab\na\nb"), dict(text=b"\n"),
               dict(text=b"\n\n\n", doc_offsets=[0, 1, 2, 3])):
        with pytest.raises(W.WordPieceError, match="even number of rows"):
            v.encode_inputs(pairs=True, max_len=8, **kw)
    for bad in ([0, 3, 3, 5], [0, 5, 3], [0, 3], [1, 3, 5], [0, 2, 5]):
        with pytest.raises(W.WordPieceError, match="document offsets"):
            v.encode_inputs(text=b"ab\na\n", doc_offsets=bad, max_len=8)
    with pytest.raises(W.WordPieceError, match="same length"):
        v.encode_inputs(a=a, b=["b"], max_len=8)
    with pytest.raises(W.WordPieceError, match="joined form"):
        v.encode_inputs(a=a, text=b"a\n", max_len=8)
    with pytest.raises(W.WordPieceError, match="a .and b. or text"):
        v.encode_inputs(max_len=8)
    # through the C ABI alone: NULL spec, unknown truncation and unit
    L = W.lib()
    text = b"ab\na\n"
    out, n, ns = W.Inputs(), C.c_size_t(), C.c_size_t()
    rc = L.wp_linear_encode_inputs(v._h, text, len(text), None, 0, None, C.byref(out), C.byref(n), C.byref(ns))
    assert rc == 6 and b"spec is NULL" in L.wp_last_error()  # WP_ERR_ARG
    for field, value, msg in (("truncation", 3, b"truncation"), ("truncation", -1, b"truncation"), ("unit", 2, b"unit"),
                              ("unit", -2, b"unit"), ("pairs", -1, b"pairs")):
        spec = W.InputsSpec(8, 1, 2, 0, 0, 0, -1, -1)
        setattr(spec, field, value)
        for t in (text, b""):
            rc = L.wp_linear_encode_inputs(v._h, t, len(t), None, 0, C.byref(spec), C.byref(out), C.byref(n), C.byref(ns))
            assert rc == 6 and msg in L.wp_last_error(), (field, value, L.wp_last_error())
            assert n.value == 0 and not out.input_ids
    # the device entry point checks the same rules before it looks for a device
    for spec, msg in ((W.InputsSpec(8, 1, 2, 0, 1, 0, 0, -1), b"windows"), (W.InputsSpec(2, 1, 2, 0, 1, 0, -1, -1), b"max_len"),
                      (W.InputsSpec(8, 1, 2, 0, 0, 2, -1, -1), b"only_second"), (W.InputsSpec(8, 1, 2, 0, 1, 1, 5, -1), b"no room")):
        rc = L.wp_linear_encode_inputs_device(v._h, None, 8, None, 0, C.byref(spec), C.byref(out), 4, C.byref(n), C.byref(ns))
        assert rc == 6 and msg in L.wp_last_error(), L.wp_last_error()
    rc = L.wp_linear_encode_inputs_device(v._h, None, 8, None, 0, None, C.byref(out), 4, C.byref(n), C.byref(ns))
    assert rc == 6 and b"spec is NULL" in L.wp_last_error()


def test_no_cpu_fallback_for_inputs():
    if W.lib().wp_device_count() > 0:
        pytest.skip("GPU present")
    v = W.Vocab(VOCAB)
    for call in (lambda: v.encode_inputs(a=["ab"], max_len=4), lambda: v.encode_inputs(a=["ab", ""], b=["", "b"], max_len=6, cls_id=1, sep_id=2),
                 lambda: v.encode_inputs(text=b"ab\nb", pairs=True, max_len=8, offsets="char"),
                 lambda: v.encode_inputs(text=b"\n", max_len=4),
                 lambda: v.encode_inputs(a=["ab a b"], max_len=2, truncation="only_first", stride=1)):
        with pytest.raises(W.WordPieceError, match="no HIP device"):
            call()


def test_mirrors_of_the_structs():
    assert [f[0] for f in W.InputsStats._fields_] == ["n_samples", "n_out", "n_cut", "n_windowed", "pairs", "truncation", "stride",
                                                     "reserved"]
    assert C.sizeof(W.InputsStats) == 48 and C.sizeof(W.InputsSpec) == 32 and C.sizeof(W.Inputs) == 5 * C.sizeof(C.c_void_p)
    assert [f[0] for f in W.InputsSpec._fields_] == ["max_len", "cls_id", "sep_id", "pad_id", "pairs", "truncation", "stride", "unit"]
    assert [f[0] for f in W.Stats._fields_][-3:] == ["n_rows", "rows_truncated", "rows_route"]  # wp_stats keeps its size and its end
    assert (W.WP_TRUNC_LONGEST_FIRST, W.WP_TRUNC_ONLY_FIRST, W.WP_TRUNC_ONLY_SECOND) == (0, 1, 2)
    for name in ("wp_linear_encode_inputs", "wp_linear_encode_inputs_device", "wp_get_inputs_stats"):
        assert name in W.ABI_SYMBOLS and hasattr(W.lib(), name)
    v = W.Vocab(VOCAB)
    assert v.inputs_stats()["n_out"] == -1  # a fresh handle: no inputs call yet
