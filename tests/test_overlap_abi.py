"""CPU checks of the overlap entry points (wp_overlap_rows, wp_overlap_rows_device, wp_get_overlap_stats): symbols and
structs against the header, what they answer without a device — every argument error with the field it names, the size
limits, bad offsets of either batch in the host form, no row, a batch without windows, the statistics before any call —
and that anything else fails loudly without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import overlap_model as M
import wordpiece_amd as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = ["[UNK]", "a", "b"]
ARG, TOO_LARGE, NO_DEVICE = 6, 2, 4
NAMES = ("wp_overlap_rows", "wp_overlap_rows_device", "wp_get_overlap_stats")
STAT_FIELDS = ["n_rows", "n_ref", "n_elems", "n_ref_elems", "n_windows", "n_ref_windows", "n_ref_distinct", "n_hits", "n_hit_rows", "n_covered",
               "n_candidates", "n_collided"]
RESULT_FIELDS = ["hits", "first_hit", "covered", "ref_hits", "row_off", "first_ref", "kept", "mask", "data", "n_rows", "n_ref", "n_kept", "n_elems"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(W.LIB_PATH):
        from wordpiece_amd import build
        build.build()


def test_symbols_and_structs_match_the_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in W.ABI_SYMBOLS and hasattr(W.lib(), name), name
    assert re.search(r"typedef struct \{ int32_t elem_bytes, want, ngram, max_hits, hash_bits, reserved\[3\]; \} wp_overlap_spec;", hdr)
    assert re.search(r"typedef struct \{ int64_t \*hits, \*first_hit, \*covered, \*ref_hits, \*row_off; int32_t \*first_ref, \*kept; uint8_t \*mask; "
                     r"void \*data; int64_t n_rows, n_ref, n_kept, n_elems; \} wp_overlap_result;", hdr)
    assert re.search(r"typedef struct \{ int64_t %s; \} wp_overlap_stats;" % ", ".join(STAT_FIELDS), hdr)
    for macro, value in (("WP_OVERLAP_WANT_MASK", 1), ("WP_OVERLAP_WANT_REF", 2), ("WP_OVERLAP_WANT_COMPACT", 4)):
        assert re.search(r"#define %s\s+%d\b" % (macro, value), hdr) and getattr(W, macro) == value
    assert [f[0] for f in W.OverlapSpec._fields_] == ["elem_bytes", "want", "ngram", "max_hits", "hash_bits", "reserved"]
    assert [f[0] for f in W.OverlapResult._fields_] == RESULT_FIELDS
    assert [(n, C.sizeof(t)) for n, t in W.OverlapStats._fields_] == [(n, 8) for n in STAT_FIELDS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(wp_stats), sizeof(wp_overlap_spec),\n'
                   '         offsetof(wp_overlap_spec, hash_bits), offsetof(wp_overlap_spec, reserved), sizeof(wp_overlap_result),\n'
                   '         offsetof(wp_overlap_result, row_off), offsetof(wp_overlap_result, first_ref), offsetof(wp_overlap_result, mask),\n'
                   '         offsetof(wp_overlap_result, data), offsetof(wp_overlap_result, n_rows), offsetof(wp_overlap_result, n_elems),\n'
                   '         sizeof(wp_overlap_stats), offsetof(wp_overlap_stats, n_collided), sizeof(wp_neardup_stats));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S, R, T = W.OverlapSpec, W.OverlapResult, W.OverlapStats
    assert got == [C.sizeof(W.Stats), C.sizeof(S), S.hash_bits.offset, S.reserved.offset, C.sizeof(R), R.row_off.offset, R.first_ref.offset,
                   R.mask.offset, R.data.offset, R.n_rows.offset, R.n_elems.offset, C.sizeof(T), T.n_collided.offset, C.sizeof(W.NearDupStats)]
    assert C.sizeof(S) == 32 and C.sizeof(R) == 104 and C.sizeof(T) == 96
    assert [f[0] for f in W.Stats._fields_][-1] == "rows_route"  # wp_stats keeps its size and its end


def _spec(elem_bytes=1, want=0, ngram=2, max_hits=0, hash_bits=0, reserved=(0, 0, 0)):
    return W.OverlapSpec(elem_bytes, want, ngram, max_hits, hash_bits, (C.c_int32 * 3)(*reserved))


def _off(values):
    return np.array(values, dtype=np.int64)


def _garbage():
    return W.OverlapResult(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13)  # (garbage in: the call clears it)


def _host(v, data, off, rdata, roff, spec, out=True, n_rows=None, n_ref=None):
    o = _garbage()
    n = (len(off) - 1 if off is not None else 0) if n_rows is None else n_rows
    nr = (len(roff) - 1 if roff is not None else 0) if n_ref is None else n_ref
    rc = W.lib().wp_overlap_rows(v._h, data, None if off is None else off.ctypes.data, n, rdata, None if roff is None else roff.ctypes.data, nr,
                                 None if spec is None else C.byref(spec), C.byref(o) if out else None)
    return rc, o


def _device(v, spec, n_rows=3, n_ref=2, out=True, data=256, off=512, rdata=1024, roff=2048):
    """the device form with pointers that are never dereferenced: the argument rules come first"""
    o = _garbage()
    rc = W.lib().wp_overlap_rows_device(v._h, C.c_void_p(data), None if off is None else C.c_void_p(off), n_rows, C.c_void_p(rdata),
                                        None if roff is None else C.c_void_p(roff), n_ref, None if spec is None else C.byref(spec),
                                        C.byref(o) if out else None)
    return rc, o


def _cleared(o):
    return not (o.hits or o.first_hit or o.covered or o.ref_hits or o.row_off or o.first_ref or o.kept or o.mask or o.data) and \
        (o.n_rows, o.n_ref, o.n_kept, o.n_elems) == (0, 0, 0, 0)


def test_argument_errors_come_before_the_device_and_name_the_field():
    L = W.lib()
    v = W.Vocab(VOCAB)
    assert v.overlap_stats()["n_rows"] == -1  # a fresh handle: no such call yet
    cases = [(None, b"spec is NULL"), (_spec(elem_bytes=0), b"elem_bytes"), (_spec(elem_bytes=2), b"elem_bytes"), (_spec(elem_bytes=-4), b"elem_bytes"),
             (_spec(want=8), b"want"), (_spec(want=-1), b"want"), (_spec(ngram=0), b"ngram"), (_spec(ngram=65), b"ngram"), (_spec(ngram=-1), b"ngram"),
             (_spec(max_hits=-1), b"max_hits"), (_spec(hash_bits=7), b"hash_bits"), (_spec(hash_bits=65), b"hash_bits"), (_spec(hash_bits=-8), b"hash_bits"),
             (_spec(reserved=(1, 0, 0)), b"reserved"), (_spec(reserved=(0, 1, 0)), b"reserved"), (_spec(reserved=(0, 0, 1)), b"reserved")]
    for spec, msg in cases:
        for data, off in ((b"abab", _off([0, 2, 4])), (b"", _off([0])), (b"", _off([0, 0]))):
            rc, o = _host(v, data, off, b"ab", _off([0, 2]), spec)
            assert rc == ARG and msg in L.wp_last_error() and _cleared(o), (msg, L.wp_last_error())
        for n_rows in (3, 0):
            rc, o = _device(v, spec, n_rows=n_rows)
            assert rc == ARG and msg in L.wp_last_error() and _cleared(o), (msg, L.wp_last_error())
    ab, o2 = b"abab", _off([0, 2, 4])
    for call in (lambda: _host(v, ab, o2, ab, o2, _spec(), out=False), lambda: _device(v, _spec(), out=False)):
        assert call()[0] == ARG and b"out is NULL" in L.wp_last_error()
    # the offsets, the data, the sizes, the alignment: each with the batch it is about
    assert _host(v, ab, None, ab, o2, _spec(), n_rows=2)[0] == ARG and b"row_off is NULL" in L.wp_last_error()
    assert _host(v, ab, o2, ab, None, _spec(), n_ref=2)[0] == ARG and b"ref_off is NULL" in L.wp_last_error()
    assert _device(v, _spec(), off=None)[0] == ARG and b"row_off is NULL" in L.wp_last_error()
    assert _device(v, _spec(), roff=None)[0] == ARG and b"ref_off is NULL" in L.wp_last_error()
    assert _host(v, None, o2, ab, o2, _spec())[0] == ARG and b"overlap: data is NULL" in L.wp_last_error()
    assert _host(v, ab, o2, None, o2, _spec())[0] == ARG and b"ref_data is NULL" in L.wp_last_error()
    assert _host(v, ab, o2, ab, o2, _spec(), n_rows=2 ** 31)[0] == TOO_LARGE and b"2^31 rows or more in row_off" in L.wp_last_error()
    assert _host(v, ab, o2, ab, o2, _spec(), n_ref=2 ** 31)[0] == TOO_LARGE and b"2^31 rows or more in ref_off" in L.wp_last_error()
    assert _device(v, _spec(), n_rows=2 ** 31)[0] == TOO_LARGE and b"in row_off" in L.wp_last_error()
    assert _device(v, _spec(), n_ref=2 ** 31)[0] == TOO_LARGE and b"in ref_off" in L.wp_last_error()
    for eb, last in ((1, 2 ** 32), (4, 2 ** 30)):
        assert _host(v, ab, _off([0, last]), ab, o2, _spec(elem_bytes=eb))[0] == TOO_LARGE and b"UINT32_MAX" in L.wp_last_error()
        assert _host(v, ab, o2, ab, _off([0, last]), _spec(elem_bytes=eb))[0] == TOO_LARGE and b"UINT32_MAX" in L.wp_last_error()
    assert _device(v, _spec(), data=257)[0] == ARG and b"overlap: data must be 4-byte aligned" in L.wp_last_error()
    assert _device(v, _spec(), rdata=1026)[0] == ARG and b"ref_data must be 4-byte aligned" in L.wp_last_error()
    assert _device(v, _spec(), off=516)[0] == ARG and b"row_off must be 8-byte aligned" in L.wp_last_error()
    assert _device(v, _spec(), roff=2052)[0] == ARG and b"ref_off must be 8-byte aligned" in L.wp_last_error()
    assert v.overlap_stats()["n_rows"] == -1  # none of these was a call


def test_bad_offsets_in_the_host_form_name_the_batch_and_the_first_bad_row():
    L = W.lib()
    v = W.Vocab(VOCAB)
    data, good = b"abcdefgh" * 4, _off([0, 4, 8])
    for off, row in (([1, 2, 3], 0), ([0, 3, 2, 8], 1), ([3, 2, 1], 0), ([0, 2, 4, 3], 2), ([0, 4, 2, 1], 1), ([-1, 2], 0), ([0, -1], 0)):
        for eb in (1, 4):
            rc, o = _host(v, data, _off(off), data, good, _spec(elem_bytes=eb))
            err = L.wp_last_error()
            assert rc == ARG and b"row_off" in err and b"ref_off" not in err and err.endswith(b"row %d" % row) and _cleared(o), (off, err)
            rc, o = _host(v, data, good, data, _off(off), _spec(elem_bytes=eb))
            err = L.wp_last_error()
            assert rc == ARG and b"ref_off" in err and b"row_off" not in err and err.endswith(b"row %d" % row) and _cleared(o), (off, err)
    # the Python mirror's own rules
    with pytest.raises(W.WordPieceError, match="end behind the data"):
        v.overlap_rows(b"abc", [0, 2, 4], b"ab", [0, 2])
    with pytest.raises(W.WordPieceError, match="ref_data end behind the data"):
        v.overlap_rows(b"abc", [0, 2, 3], b"ab", [0, 3])
    with pytest.raises(W.WordPieceError, match="n_rows \\+ 1"):
        v.overlap_rows(b"abc", [], b"ab", [0, 2])
    with pytest.raises(W.WordPieceError, match="text .* or a flat int32"):
        v.overlap_rows(np.zeros(3, dtype=np.int64), [0, 3], b"ab", [0, 2])
    with pytest.raises(W.WordPieceError, match="both be text or both be ids"):
        v.overlap_rows(np.zeros(3, dtype=np.int32), [0, 3], b"ab", [0, 2])
    with pytest.raises(W.WordPieceError, match="ref_off"):
        v.overlap_rows(b"abc", [0, 3], b"abc", [0, 2, 1])
    with pytest.raises(W.WordPieceError, match="ngram"):
        v.overlap_rows(b"abc", [0, 3], b"abc", [0, 3], ngram=0)
    assert v.overlap_stats()["n_rows"] == -1


def test_no_row_needs_no_device():
    L = W.lib()
    v = W.Vocab(VOCAB)
    for eb in (1, 4):
        for want in range(8):
            rc, o = _host(v, None, _off([0]), b"abab", _off([0, 1, 4]), _spec(eb, want, ngram=1))
            assert rc == 0 and not (o.hits or o.first_hit or o.covered or o.ref_hits or o.row_off or o.first_ref or o.kept or o.mask or o.data)
            assert (o.n_rows, o.n_ref, o.n_kept, o.n_elems) == (0, 2, 0, 0)
            st = v.overlap_stats()
            assert st["n_rows"] == 0 and st["n_ref"] == 2 and all(st[k] == 0 for k in STAT_FIELDS[2:])
            rc, o = _device(v, _spec(eb, want), n_rows=0, data=0, off=0)
            assert rc == 0 and (o.n_rows, o.n_ref, o.n_kept, o.n_elems) == (0, 2, 0, 0) and not (o.hits or o.kept or o.row_off or o.data)
    r = v.overlap_rows(b"", None, b"ab\ncd\n", None, ngram=2, mask=True, ref=True, compact=True)  # the lines of the empty text: no line
    assert all(r[k].shape == (0,) for k in ("hits", "first_hit", "first_ref", "covered", "mask", "kept")) and r["ref_hits"].shape == (0,)
    assert r["data"] == b"" and r["row_off"].tolist() == [0]
    assert v.overlap_docs([], ["ab"])[0] == [] and v.overlap_docs([], ["ab"])[1].shape == (0,)


def _same(got, exp, st, eb):
    for key, dtype in (("hits", np.int64), ("first_hit", np.int64), ("first_ref", np.int32), ("covered", np.int64), ("mask", np.uint8),
                       ("ref_hits", np.int64), ("kept", np.int32), ("row_off", np.int64)):
        assert got[key].dtype == dtype and got[key].tolist() == exp[key], key
    data = got["data"] if eb == 1 else got["data"].tobytes()
    assert data == exp["data"] and {k: st[k] for k in exp["stats"]} == exp["stats"] and st["n_candidates"] == st["n_collided"] == 0


def test_a_batch_without_windows_needs_no_device():
    v = W.Vocab(VOCAB)
    ids = np.arange(1, 9, dtype=np.int32)
    cases = [  # (corpus rows, reference rows, k): short corpus rows, short reference rows, no reference row, empty rows only
        ([b"ab", b"", b"abc"], [b"abcd", b"abcd", b"xyzw"], 4), ([b"abcdef", b"abc"], [b"ab", b"", b"c"], 3), ([b"abcdef", b""], [], 2),
        ([b"", b""], [b"aaaa"], 1), ([b"abc"], [b""], 1)]
    for rows, refs, k in cases:
        for eb in (1, 4):
            if eb == 4:
                rows4, refs4 = [ids[:len(r)].tobytes() for r in rows], [ids[:len(r)].tobytes() for r in refs]
            data, off = M.join(rows4 if eb == 4 else rows, eb)
            rdata, roff = M.join(refs4 if eb == 4 else refs, eb)
            for max_hits in (0, 3):
                exp = M.overlap_rows(data, off, rdata, roff, elem_bytes=eb, ngram=k, max_hits=max_hits)
                arr = (lambda b: b) if eb == 1 else (lambda b: np.frombuffer(b, dtype=np.int32))
                got = v.overlap_rows(arr(data), off, arr(rdata), roff, ngram=k, max_hits=max_hits, mask=True, ref=True, compact=True)
                _same(got, exp, v.overlap_stats(), eb)
                assert exp["stats"]["n_hits"] == 0 and exp["kept"] == list(range(len(rows)))
                plain = v.overlap_rows(arr(data), off, arr(rdata), roff, ngram=k)
                assert sorted(plain) == ["covered", "first_hit", "first_ref", "hits"] and plain["first_hit"].tolist() == [-1] * len(rows)
    assert v.overlap_docs(["ab", "c"], ["abcdefgh"], ngram=5)[0] == ["ab", "c"]


def test_no_cpu_fallback():
    if W.lib().wp_device_count() > 0:
        pytest.skip("GPU present")
    v = W.Vocab(VOCAB)
    L = W.lib()
    for data, off in ((b"abab", [0, 2, 4]), (b"ab", [0, 0, 2])):
        rc, o = _host(v, data, _off(off), b"xab", _off([0, 3]), _spec())
        assert rc == NO_DEVICE and b"no HIP device" in L.wp_last_error() and _cleared(o)
    assert _device(v, _spec())[0] == NO_DEVICE and b"no HIP device" in L.wp_last_error()
    with pytest.raises(W.WordPieceError, match="no HIP device"):
        v.overlap_rows(b"ab\ncd\n", None, b"cd\n", None, ngram=2)
    with pytest.raises(W.WordPieceError, match="no HIP device"):
        v.overlap_docs(["abc", "bcd"], ["xbc"], ngram=2)
