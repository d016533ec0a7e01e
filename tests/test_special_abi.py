"""CPU checks of the special-tokens entry points (wp_linear_encode_special, its documents and device forms,
wp_get_special_stats): symbols and structs against the header, what the host entry points answer without a device —
every argument error with the id it names, empty texts — and that anything else fails loudly without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import special_model as S
import wordpiece_amd as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = ["[UNK]", "a", "[MASK]", "[.]", "[MASK]", "[a b]", "##[x]", "[" + "y" * 62 + "]", "[" + "y" * 63 + "]", "[é]", "[a[b]", "[SEP]",
         "[a]b]", "[]"]
ARG, TOO_LARGE, NO_DEVICE = 6, 2, 4
NAMES = ("wp_linear_encode_special", "wp_linear_encode_special_device", "wp_linear_encode_special_rows",
         "wp_linear_encode_special_rows_device", "wp_get_special_stats")


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(W.LIB_PATH):
        from wordpiece_amd import build
        build.build()


def test_symbols_and_structs_match_the_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in W.ABI_SYMBOLS and hasattr(W.lib(), name), name
    assert "add_special_tokens" in hdr and "all_special_ids" in hdr
    assert re.search(r"typedef struct \{ const int32_t \*ids; int32_t n_ids; \} wp_special_spec;", hdr)
    assert re.search(r"typedef struct \{ int64_t n_literals, n_ids, n_rows, n_listed; \} wp_special_stats;", hdr)
    assert [f[0] for f in W.SpecialSpec._fields_] == ["ids", "n_ids"]
    assert [(n, C.sizeof(t)) for n, t in W.SpecialStats._fields_] == [("n_literals", 8), ("n_ids", 8), ("n_rows", 8), ("n_listed", 8)]
    assert [f[0] for f in W.Stats._fields_][-1] == "rows_route"  # wp_stats keeps its size and its end
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(wp_stats), sizeof(wp_special_spec), offsetof(wp_special_spec, n_ids),\n'
                   '         sizeof(wp_special_stats), offsetof(wp_special_stats, n_rows), offsetof(wp_special_stats, n_listed));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(W.Stats), C.sizeof(W.SpecialSpec), W.SpecialSpec.n_ids.offset, C.sizeof(W.SpecialStats),
                   W.SpecialStats.n_rows.offset, W.SpecialStats.n_listed.offset]
    assert C.sizeof(W.SpecialStats) == 32


def _spec(ids):
    a = np.ascontiguousarray(ids, dtype=np.int32)
    return W.SpecialSpec(W._i32_ptr(a) if len(a) else None, len(a)), a


def _flat(v, text, spec, unit=0, offsets=True):
    ids, offs, n = C.POINTER(C.c_int32)(), C.POINTER(C.c_uint32)(), C.c_size_t(77)
    rc = W.lib().wp_linear_encode_special(v._h, text, len(text), None if spec is None else C.byref(spec), unit, C.byref(ids),
                                          C.byref(offs) if offsets else None, C.byref(n))
    return rc, bool(ids), bool(offs), n.value


def _rows(v, text, doc_off, spec, unit=0):
    ids, splits, offs = C.POINTER(C.c_int32)(), C.POINTER(C.c_int64)(), C.POINTER(C.c_uint32)()
    n, rows = C.c_size_t(77), C.c_size_t(77)
    off = None if doc_off is None else np.ascontiguousarray(doc_off, dtype=np.int64)
    rc = W.lib().wp_linear_encode_special_rows(v._h, text, len(text), W._i64_ptr(off), 0 if off is None else len(off) - 1,
                                               None if spec is None else C.byref(spec), unit, C.byref(ids), C.byref(splits),
                                               C.byref(offs), C.byref(n), C.byref(rows))
    sp = None
    if splits:
        sp = [splits[i] for i in range(rows.value + 1)]
        W.lib().wp_free(splits)
    return rc, bool(ids), sp, n.value, rows.value


def _device_calls(v, spec, unit=0):
    """the device forms with pointers that are never dereferenced: the argument rules come first"""
    L = W.lib()
    dev, a, b, c, n, r = C.c_void_p(256), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
    sp = None if spec is None else C.byref(spec)
    return (L.wp_linear_encode_special_device(v._h, dev, 8, sp, unit, C.byref(a), C.byref(b), C.byref(n)),
            L.wp_linear_encode_special_rows_device(v._h, dev, 8, None, 0, sp, unit, C.byref(a), C.byref(c), C.byref(b), C.byref(n),
                                                   C.byref(r)))


def test_list_errors_come_before_the_device_and_name_the_id():
    L = W.lib()
    v = W.Vocab(VOCAB)
    assert v.special_stats()["n_literals"] == -1  # a fresh handle: no such call yet
    text = b"a [MASK] a\n"
    cases = [([14], b"id 14 "), ([-1], b"id -1 "), ([1], b"id 1 "), ([3], b"id 3 "), ([5], b"id 5 "), ([6], b"id 6 "),
             ([8], b"id 8 "), ([9], b"id 9 "), ([10], b"id 10 "), ([12], b"id 12 "), ([13], b"id 13 "), ([2, 4], b"id 4 "),
             ([4, 11, 2], b"id 4 "), ([0, 2, 99], b"id 99 ")]
    for ids, msg in cases:
        with pytest.raises(ValueError):  # the model refuses the same lists
            S.table(VOCAB, ids)
        spec, keep = _spec(ids)
        for rc, any_ids, any_offs, n in (_flat(v, text, spec), _flat(v, b"", spec)):
            assert rc == ARG and msg in L.wp_last_error() and not any_ids and not any_offs and n == 0, (ids, L.wp_last_error())
        for doc_off in (None, [0, 11]):
            rc, any_ids, sp, n, rows = _rows(v, text, doc_off, spec)
            assert rc == ARG and msg in L.wp_last_error() and not any_ids and sp is None and n == 0 and rows == 0, (ids, L.wp_last_error())
        for rc in _device_calls(v, spec):
            assert rc == ARG and msg in L.wp_last_error(), (ids, L.wp_last_error())
    # the spec itself
    for spec, msg in ((None, b"spec is NULL"), (W.SpecialSpec(None, 1), b"ids is NULL"), (W.SpecialSpec(None, -1), b"n_ids"),
                      (_spec([2] * 4097)[0], b"n_ids")):
        assert _flat(v, text, spec)[0] == ARG and msg in L.wp_last_error()
        assert _rows(v, text, None, spec)[0] == ARG and msg in L.wp_last_error()
        for rc in _device_calls(v, spec):
            assert rc == ARG and msg in L.wp_last_error()
    # the unit, the place for offsets, the documents, the size
    spec, keep = _spec([2, 0, 2, 7, 11])
    S.table(VOCAB, [2, 0, 2, 7, 11])
    for unit in (2, -2):
        assert _flat(v, text, spec, unit)[0] == ARG and b"unit" in L.wp_last_error()
        assert _rows(v, text, None, spec, unit)[0] == ARG and b"unit" in L.wp_last_error()
        assert all(rc == ARG for rc in _device_calls(v, spec, unit))
    assert _flat(v, text, spec, 0, offsets=False)[0] == ARG and b"offsets" in L.wp_last_error()
    assert _rows(v, text, [0, 5], spec)[0] == ARG and b"document offsets" in L.wp_last_error()
    assert _rows(v, text, [0, 3, 11], spec)[0] == ARG and b"document offsets" in L.wp_last_error()
    ids, offs, n = C.POINTER(C.c_int32)(), C.POINTER(C.c_uint32)(), C.c_size_t()
    rc = L.wp_linear_encode_special(v._h, text, 2 ** 32, C.byref(spec), -1, C.byref(ids), C.byref(offs), C.byref(n))
    assert rc == TOO_LARGE and b"UINT32_MAX" in L.wp_last_error()
    assert v.special_stats()["n_literals"] == -1  # none of these was a call


def test_empty_text_needs_no_device():
    v = W.Vocab(VOCAB)
    spec, keep = _spec([2, 11, 2])
    for unit in (-1, 0, 1):
        assert _flat(v, b"", spec, unit) == (0, False, False, 0)
        assert v.special_stats() == dict(n_literals=0, n_ids=0, n_rows=-1, n_listed=3)
        assert _rows(v, b"", None, spec, unit) == (0, False, [0], 0, 0)
        assert v.special_stats() == dict(n_literals=0, n_ids=0, n_rows=0, n_listed=3)
        assert _rows(v, b"\n\n\n", [0, 1, 2, 3], spec, unit) == (0, False, [0, 0, 0, 0], 0, 3)
        assert v.special_stats() == dict(n_literals=0, n_ids=0, n_rows=3, n_listed=3)
    assert _flat(v, b"", _spec([])[0], -1, offsets=False) == (0, False, False, 0)
    # the Python mirror
    assert v.encode_special("").tolist() == [] and v.encode_special("", offsets="char")[1].shape == (0, 2)
    ids, splits = v.encode_special_rows(docs=["", ""], special_ids=[])
    assert ids.tolist() == [] and splits.tolist() == [0, 0, 0]
    assert v.special_ids() == [0, 2, 7, 11] == S.special_ids(VOCAB)
    assert v.special_ids(["[SEP]", "[MASK]"]) == [11, 2] == S.special_ids(VOCAB, ["[SEP]", "[MASK]"])
    for bad in ("[.]", "a", "[a b]", "[nope]", "##[x]"):
        with pytest.raises(W.WordPieceError, match="no special token"):
            v.special_ids([bad])


def test_no_cpu_fallback():
    if W.lib().wp_device_count() > 0:
        pytest.skip("GPU present")
    v = W.Vocab(VOCAB)
    spec, keep = _spec([2])
    L = W.lib()
    for text in (b"a [MASK] a", b"a a"):
        assert _flat(v, text, spec)[0] == NO_DEVICE and b"no HIP device" in L.wp_last_error()
        assert _rows(v, text + b"\n", None, spec)[0] == NO_DEVICE and b"no HIP device" in L.wp_last_error()
    assert _flat(v, b"a", _spec([])[0])[0] == NO_DEVICE
    with pytest.raises(W.WordPieceError, match="no HIP device"):
        v.encode_special("a [MASK]")
    with pytest.raises(W.WordPieceError, match="no HIP device"):
        v.encode_special_rows(docs=["a [MASK]"], offsets="byte")
