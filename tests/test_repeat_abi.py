"""CPU checks of the repeat entry points (wp_repeat_rows, wp_repeat_rows_device, wp_get_repeat_stats): symbols and structs
against the header, what they answer without a device — every argument error with the field it names, the size limits,
bad offsets in the host form, no row, a batch without windows, the statistics before any call — and that anything else
fails loudly without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import repeat_model as M
import wordpiece_amd as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = ["[UNK]", "a", "b"]
ARG, TOO_LARGE, NO_DEVICE = 6, 2, 4
NAMES = ("wp_repeat_rows", "wp_repeat_rows_device", "wp_get_repeat_stats")
STAT_FIELDS = ["n_rows", "n_elems", "n_windows", "n_distinct", "n_repeats", "n_repeat_rows", "n_covered", "n_cut_elems", "n_collided"]
SPEC_FIELDS = ["elem_bytes", "want", "ngram", "scope", "max_repeats", "hash_bits", "flags", "reserved"]
RESULT_FIELDS = ["repeats", "first_repeat", "first_src_pos", "covered", "src", "row_off", "cut_off", "first_src_row", "kept", "mask", "data", "cut_data",
                 "n_rows", "n_kept", "n_elems", "n_cut_elems"]
POINTERS = RESULT_FIELDS[:12]


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(W.LIB_PATH):
        from wordpiece_amd import build
        build.build()


def test_symbols_and_structs_match_the_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in W.ABI_SYMBOLS and hasattr(W.lib(), name), name
    assert re.search(r"typedef struct \{ int32_t %s; \} wp_repeat_spec;" % ", ".join(SPEC_FIELDS), hdr)
    assert re.search(r"typedef struct \{ int64_t \*repeats, \*first_repeat, \*first_src_pos, \*covered, \*src, \*row_off, \*cut_off; "
                     r"int32_t \*first_src_row, \*kept; uint8_t \*mask; void \*data, \*cut_data; int64_t n_rows, n_kept, n_elems, n_cut_elems; \} "
                     r"wp_repeat_result;", hdr)
    assert re.search(r"typedef struct \{ int64_t %s; \} wp_repeat_stats;" % ", ".join(STAT_FIELDS), hdr)
    for macro, value in (("WP_REPEAT_WANT_MASK", 1), ("WP_REPEAT_WANT_SRC", 2), ("WP_REPEAT_WANT_COMPACT", 4), ("WP_REPEAT_WANT_CUT", 8),
                         ("WP_REPEAT_UTF8", 1)):
        assert re.search(r"#define %s\s+%d\b" % (macro, value), hdr) and getattr(W, macro) == value
    assert [f[0] for f in W.RepeatSpec._fields_] == SPEC_FIELDS
    assert [f[0] for f in W.RepeatResult._fields_] == RESULT_FIELDS
    assert [(n, C.sizeof(t)) for n, t in W.RepeatStats._fields_] == [(n, 8) for n in STAT_FIELDS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(wp_stats), sizeof(wp_repeat_spec),\n'
                   '         offsetof(wp_repeat_spec, hash_bits), offsetof(wp_repeat_spec, reserved), sizeof(wp_repeat_result),\n'
                   '         offsetof(wp_repeat_result, cut_off), offsetof(wp_repeat_result, first_src_row), offsetof(wp_repeat_result, mask),\n'
                   '         offsetof(wp_repeat_result, cut_data), offsetof(wp_repeat_result, n_rows), offsetof(wp_repeat_result, n_cut_elems),\n'
                   '         sizeof(wp_repeat_stats), offsetof(wp_repeat_stats, n_collided), sizeof(wp_overlap_stats));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S, R, T = W.RepeatSpec, W.RepeatResult, W.RepeatStats
    assert got == [C.sizeof(W.Stats), C.sizeof(S), S.hash_bits.offset, S.reserved.offset, C.sizeof(R), R.cut_off.offset, R.first_src_row.offset,
                   R.mask.offset, R.cut_data.offset, R.n_rows.offset, R.n_cut_elems.offset, C.sizeof(T), T.n_collided.offset, C.sizeof(W.OverlapStats)]
    assert C.sizeof(S) == 32 and C.sizeof(R) == 128 and C.sizeof(T) == 72
    assert [f[0] for f in W.Stats._fields_][-1] == "rows_route"  # wp_stats keeps its size and its end


def _spec(elem_bytes=1, want=0, ngram=2, scope=0, max_repeats=0, hash_bits=0, flags=0, reserved=0):
    return W.RepeatSpec(elem_bytes, want, ngram, scope, max_repeats, hash_bits, flags, reserved)


def _off(values):
    return np.array(values, dtype=np.int64)


def _garbage():
    return W.RepeatResult(*range(1, 17))  # (garbage in: the call clears it)


def _host(v, data, off, spec, out=True, n_rows=None):
    o = _garbage()
    n = (len(off) - 1 if off is not None else 0) if n_rows is None else n_rows
    rc = W.lib().wp_repeat_rows(v._h, data, None if off is None else off.ctypes.data, n, None if spec is None else C.byref(spec), C.byref(o) if out else None)
    return rc, o


def _device(v, spec, n_rows=3, out=True, data=256, off=512):
    """the device form with pointers that are never dereferenced: the argument rules come first"""
    o = _garbage()
    rc = W.lib().wp_repeat_rows_device(v._h, C.c_void_p(data), None if off is None else C.c_void_p(off), n_rows, None if spec is None else C.byref(spec),
                                       C.byref(o) if out else None)
    return rc, o


def _cleared(o):
    return not any(getattr(o, k) for k in RESULT_FIELDS)


def _free(o):
    for k in POINTERS:
        if getattr(o, k):
            W.lib().wp_free(getattr(o, k))


def test_argument_errors_come_before_the_device_and_name_the_field():
    L = W.lib()
    v = W.Vocab(VOCAB)
    assert v.repeat_stats()["n_rows"] == -1  # a fresh handle: no such call yet
    cases = [(None, b"spec is NULL"), (_spec(elem_bytes=0), b"elem_bytes"), (_spec(elem_bytes=2), b"elem_bytes"), (_spec(elem_bytes=-4), b"elem_bytes"),
             (_spec(want=16), b"want"), (_spec(want=-1), b"want"), (_spec(ngram=0), b"ngram"), (_spec(ngram=65), b"ngram"), (_spec(ngram=-1), b"ngram"),
             (_spec(scope=2), b"scope"), (_spec(scope=-1), b"scope"), (_spec(max_repeats=-1), b"max_repeats"), (_spec(hash_bits=7), b"hash_bits"),
             (_spec(hash_bits=65), b"hash_bits"), (_spec(hash_bits=-8), b"hash_bits"), (_spec(flags=2), b"flags"), (_spec(flags=-1), b"flags"),
             (_spec(elem_bytes=4, flags=1), b"flags"), (_spec(reserved=1), b"reserved"), (_spec(reserved=-1), b"reserved")]
    for spec, msg in cases:
        for data, off in ((b"abab", _off([0, 2, 4])), (b"", _off([0])), (b"", _off([0, 0]))):
            rc, o = _host(v, data, off, spec)
            assert rc == ARG and msg in L.wp_last_error() and L.wp_last_error().startswith(b"repeat: ") and _cleared(o), (msg, L.wp_last_error())
        for n_rows in (3, 0):
            rc, o = _device(v, spec, n_rows=n_rows)
            assert rc == ARG and msg in L.wp_last_error() and _cleared(o), (msg, L.wp_last_error())
    ab, o2 = b"abab", _off([0, 2, 4])
    for call in (lambda: _host(v, ab, o2, _spec(), out=False), lambda: _device(v, _spec(), out=False)):
        assert call()[0] == ARG and b"out is NULL" in L.wp_last_error()
    assert _host(v, ab, None, _spec(), n_rows=2)[0] == ARG and b"row_off is NULL" in L.wp_last_error()
    assert _device(v, _spec(), off=None)[0] == ARG and b"row_off is NULL" in L.wp_last_error()
    assert _host(v, None, o2, _spec())[0] == ARG and b"repeat: data is NULL" in L.wp_last_error()
    assert _host(v, ab, o2, _spec(), n_rows=2 ** 31)[0] == TOO_LARGE and b"2^31 rows or more in row_off" in L.wp_last_error()
    assert _device(v, _spec(), n_rows=2 ** 31)[0] == TOO_LARGE and b"in row_off" in L.wp_last_error()
    for eb, last in ((1, 2 ** 32), (4, 2 ** 30)):
        assert _host(v, ab, _off([0, last]), _spec(elem_bytes=eb))[0] == TOO_LARGE and b"UINT32_MAX" in L.wp_last_error()
    assert _device(v, _spec(), data=257)[0] == ARG and b"repeat: data must be 4-byte aligned" in L.wp_last_error()
    assert _device(v, _spec(), off=516)[0] == ARG and b"row_off must be 8-byte aligned" in L.wp_last_error()
    assert v.repeat_stats()["n_rows"] == -1  # none of these was a call


def test_bad_offsets_in_the_host_form_name_the_first_bad_row():
    L = W.lib()
    v = W.Vocab(VOCAB)
    data = b"abcdefgh" * 4
    for off, row in (([1, 2, 3], 0), ([0, 3, 2, 8], 1), ([3, 2, 1], 0), ([0, 2, 4, 3], 2), ([0, 4, 2, 1], 1), ([-1, 2], 0), ([0, -1], 0)):
        for eb in (1, 4):
            rc, o = _host(v, data, _off(off), _spec(elem_bytes=eb))
            err = L.wp_last_error()
            assert rc == ARG and b"row_off" in err and err.endswith(b"row %d" % row) and _cleared(o), (off, err)
    # the Python mirror's own rules
    with pytest.raises(W.WordPieceError, match="end behind the data"):
        v.repeat_rows(b"abc", [0, 2, 4])
    with pytest.raises(W.WordPieceError, match="n_rows \\+ 1"):
        v.repeat_rows(b"abc", [])
    with pytest.raises(W.WordPieceError, match="text .* or a flat int32"):
        v.repeat_rows(np.zeros(3, dtype=np.int64), [0, 3])
    with pytest.raises(W.WordPieceError, match="row_off"):
        v.repeat_rows(b"abc", [0, 2, 1])
    with pytest.raises(W.WordPieceError, match="ngram"):
        v.repeat_rows(b"abc", [0, 3], ngram=0)
    with pytest.raises(W.WordPieceError, match="flags"):
        v.repeat_rows(np.zeros(3, dtype=np.int32), [0, 3], ngram=2, utf8=True)
    with pytest.raises(W.WordPieceError, match="lines form takes no offsets"):
        v.repeat_rows(b"abc", [0, 3], lines=True)
    assert v.repeat_stats()["n_rows"] == -1


def test_no_row_needs_no_device():
    v = W.Vocab(VOCAB)
    for eb in (1, 4):
        for want in range(16):
            rc, o = _host(v, None, _off([0]), _spec(eb, want, ngram=1))
            assert rc == 0 and _cleared(o)
            st = v.repeat_stats()
            assert all(st[k] == 0 for k in STAT_FIELDS)
            rc, o = _device(v, _spec(eb, want), n_rows=0, data=0, off=0)
            assert rc == 0 and _cleared(o)
    r = v.repeat_rows(b"", None, ngram=2, mask=True, src=True, compact=True, cut=True, lines=True)  # the lines of the empty text: no line
    assert all(r[k].shape == (0,) for k in ("repeats", "first_repeat", "first_src_row", "first_src_pos", "covered", "mask", "src", "kept"))
    assert r["data"] == b"" and r["cut_data"] == b"" and r["row_off"].tolist() == [0] and r["cut_off"].tolist() == [0]
    assert v.repeat_docs([])[0] == [] and v.repeat_docs([])[1].shape == (0,)


def test_a_batch_without_windows_needs_no_device():
    v = W.Vocab(VOCAB)
    ids = np.arange(1, 9, dtype=np.int32)
    for rows, k in (([b"ab", b"", b"abc"], 4), ([b"", b""], 1), ([b"abcdef"], 7), ([b"aaa", b"aaa", b"aaa"], 4)):
        for eb in (1, 4):
            data, off = M.join([ids[:len(r)].tobytes() for r in rows] if eb == 4 else rows, eb)
            arr = data if eb == 1 else np.frombuffer(data, dtype=np.int32)
            for scope in (0, 1):
                exp = M.repeat_rows(data, off, elem_bytes=eb, ngram=k, scope=scope, max_repeats=scope)
                got = v.repeat_rows(arr, off, ngram=k, scope=scope, max_repeats=scope, mask=True, src=True, compact=True, cut=True, utf8=False)
                for key, dtype in (("repeats", np.int64), ("first_repeat", np.int64), ("first_src_row", np.int32), ("first_src_pos", np.int64),
                                   ("covered", np.int64), ("mask", np.uint8), ("src", np.int64), ("kept", np.int32), ("row_off", np.int64),
                                   ("cut_off", np.int64)):
                    assert got[key].dtype == dtype and got[key].tolist() == exp[key], key
                for key in ("data", "cut_data"):
                    assert (got[key] if eb == 1 else got[key].tobytes()) == exp[key] == data, key
                st = v.repeat_stats()
                assert {k_: st[k_] for k_ in exp["stats"]} == exp["stats"] and st["n_collided"] == 0 and st["n_windows"] == 0
                plain = v.repeat_rows(arr, off, ngram=k)
                assert sorted(plain) == ["covered", "first_repeat", "first_src_pos", "first_src_row", "repeats"] and plain["first_repeat"].tolist() == [-1] * len(rows)
                assert v.repeat_stats()["n_cut_elems"] == 0
    docs, covered = v.repeat_docs(["ab", b"c", "ab"], ngram=5)
    assert docs == ["ab", b"c", "ab"] and covered.tolist() == [0, 0, 0]


def test_no_cpu_fallback():
    if W.lib().wp_device_count() > 0:
        pytest.skip("GPU present")
    v = W.Vocab(VOCAB)
    L = W.lib()
    for data, off in ((b"abab", [0, 2, 4]), (b"ab", [0, 0, 2])):
        rc, o = _host(v, data, _off(off), _spec())
        assert rc == NO_DEVICE and b"no HIP device" in L.wp_last_error() and _cleared(o)
    assert _device(v, _spec())[0] == NO_DEVICE and b"no HIP device" in L.wp_last_error()
    with pytest.raises(W.WordPieceError, match="no HIP device"):
        v.repeat_rows(b"ab\ncd\n", None, ngram=2)
    with pytest.raises(W.WordPieceError, match="no HIP device"):
        v.repeat_docs(["abc", "bcd"], ngram=2)
