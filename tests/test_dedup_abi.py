"""CPU checks of the dedup entry points (wp_dedup_rows, wp_dedup_rows_device, wp_get_dedup_stats): symbols and structs
against the header, what they answer without a device — every argument error with the field it names, bad offsets in the
host form, no row, rows that are all empty, the statistics before any call — and that anything else fails loudly
without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dedup_model as DM
import wordpiece_amd as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = ["[UNK]", "a", "b"]
ARG, TOO_LARGE, NO_DEVICE = 6, 2, 4
NAMES = ("wp_dedup_rows", "wp_dedup_rows_device", "wp_get_dedup_stats")
STAT_FIELDS = ["n_rows", "n_unique", "n_empty", "n_elems", "n_chunks", "n_compared", "n_rounds", "n_collided"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(W.LIB_PATH):
        from wordpiece_amd import build
        build.build()


def test_symbols_and_structs_match_the_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in W.ABI_SYMBOLS and hasattr(W.lib(), name), name
    assert re.search(r"typedef struct \{ int32_t elem_bytes, want, hash_bits, reserved; \} wp_dedup_spec;", hdr)
    assert re.search(r"typedef struct \{ int32_t \*first, \*kept, \*inverse; int64_t \*counts, \*row_off; void \*data; int64_t n_rows, "
                     r"n_unique, n_elems; \} wp_dedup_result;", hdr)
    assert re.search(r"typedef struct \{ int64_t %s; \} wp_dedup_stats;" % ", ".join(STAT_FIELDS), hdr)
    for macro, value in (("WP_DEDUP_WANT_INVERSE", 1), ("WP_DEDUP_WANT_COMPACT", 2)):
        assert re.search(r"#define %s\s+%d\b" % (macro, value), hdr) and getattr(W, macro) == value
    assert [f[0] for f in W.DedupSpec._fields_] == ["elem_bytes", "want", "hash_bits", "reserved"]
    assert [f[0] for f in W.DedupResult._fields_] == ["first", "kept", "inverse", "counts", "row_off", "data", "n_rows", "n_unique", "n_elems"]
    assert [(n, C.sizeof(t)) for n, t in W.DedupStats._fields_] == [(n, 8) for n in STAT_FIELDS]
    assert [f[0] for f in W.Stats._fields_][-1] == "rows_route"  # wp_stats keeps its size and its end
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(wp_stats), sizeof(wp_dedup_spec),\n'
                   '         offsetof(wp_dedup_spec, hash_bits), sizeof(wp_dedup_result), offsetof(wp_dedup_result, inverse),\n'
                   '         offsetof(wp_dedup_result, counts), offsetof(wp_dedup_result, data), offsetof(wp_dedup_result, n_rows),\n'
                   '         offsetof(wp_dedup_result, n_elems), sizeof(wp_dedup_stats), offsetof(wp_dedup_stats, n_collided));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    R = W.DedupResult
    assert got == [C.sizeof(W.Stats), C.sizeof(W.DedupSpec), W.DedupSpec.hash_bits.offset, C.sizeof(R), R.inverse.offset, R.counts.offset,
                   R.data.offset, R.n_rows.offset, R.n_elems.offset, C.sizeof(W.DedupStats), W.DedupStats.n_collided.offset]
    assert C.sizeof(W.DedupSpec) == 16 and C.sizeof(R) == 72 and C.sizeof(W.DedupStats) == 64
    # wp_stats is the size it was before this section came (the learner's test pins the same number through its own probe)
    assert C.sizeof(W.Stats) == got[0]


def _spec(elem_bytes=1, want=0, hash_bits=0, reserved=0):
    return W.DedupSpec(elem_bytes, want, hash_bits, reserved)


def _off(values):
    return np.array(values, dtype=np.int64)


def _host(v, data, off, spec, out=True, n_rows=None):
    o = W.DedupResult(1, 2, 3, 4, 5, 6, 7, 8, 9)  # (garbage in: the call clears it)
    n = (len(off) - 1 if off is not None else 0) if n_rows is None else n_rows
    rc = W.lib().wp_dedup_rows(v._h, data, None if off is None else off.ctypes.data, n, None if spec is None else C.byref(spec),
                               C.byref(o) if out else None)
    return rc, o


def _device(v, spec, n_rows=3, out=True, data=256, off=512):
    """the device form with pointers that are never dereferenced: the argument rules come first"""
    o = W.DedupResult(1, 2, 3, 4, 5, 6, 7, 8, 9)
    rc = W.lib().wp_dedup_rows_device(v._h, C.c_void_p(data), None if off is None else C.c_void_p(off), n_rows,
                                      None if spec is None else C.byref(spec), C.byref(o) if out else None)
    return rc, o


def _cleared(o):
    return not (o.first or o.kept or o.inverse or o.counts or o.row_off or o.data) and (o.n_rows, o.n_unique, o.n_elems) == (0, 0, 0)


def test_argument_errors_come_before_the_device_and_name_the_field():
    L = W.lib()
    v = W.Vocab(VOCAB)
    assert v.dedup_stats()["n_rows"] == -1  # a fresh handle: no such call yet
    cases = [(None, b"spec is NULL"), (_spec(elem_bytes=0), b"elem_bytes"), (_spec(elem_bytes=2), b"elem_bytes"), (_spec(elem_bytes=8), b"elem_bytes"),
             (_spec(elem_bytes=-1), b"elem_bytes"), (_spec(want=4), b"want"), (_spec(want=-1), b"want"), (_spec(hash_bits=7), b"hash_bits"),
             (_spec(hash_bits=65), b"hash_bits"), (_spec(hash_bits=-1), b"hash_bits"), (_spec(reserved=1), b"reserved")]
    for spec, msg in cases:
        for data, off in ((b"abab", _off([0, 2, 4])), (b"", _off([0])), (b"", _off([0, 0]))):
            rc, o = _host(v, data, off, spec)
            assert rc == ARG and msg in L.wp_last_error() and _cleared(o), (msg, L.wp_last_error())
        for n_rows in (3, 0):
            rc, o = _device(v, spec, n_rows=n_rows)
            assert rc == ARG and msg in L.wp_last_error() and _cleared(o), (msg, L.wp_last_error())
    for call in (lambda: _host(v, b"a", _off([0, 1]), _spec(), out=False), lambda: _device(v, _spec(), out=False)):
        assert call()[0] == ARG and b"out is NULL" in L.wp_last_error()
    # row_off, data, the sizes, the alignment
    assert _host(v, b"ab", None, _spec(), n_rows=2)[0] == ARG and b"row_off is NULL" in L.wp_last_error()
    assert _device(v, _spec(), off=None)[0] == ARG and b"row_off is NULL" in L.wp_last_error()
    assert _host(v, None, _off([0, 1]), _spec())[0] == ARG and b"data is NULL" in L.wp_last_error()
    assert _host(v, b"a", _off([0, 1]), _spec(), n_rows=2 ** 31)[0] == TOO_LARGE and b"2^31 rows" in L.wp_last_error()
    assert _device(v, _spec(), n_rows=2 ** 31)[0] == TOO_LARGE and b"2^31 rows" in L.wp_last_error()
    assert _host(v, b"a", _off([0, 2 ** 32]), _spec())[0] == TOO_LARGE and b"UINT32_MAX" in L.wp_last_error()
    assert _host(v, b"a", _off([0, 2 ** 30]), _spec(elem_bytes=4))[0] == TOO_LARGE and b"UINT32_MAX" in L.wp_last_error()
    assert _device(v, _spec(), data=257)[0] == ARG and b"data must be 4-byte aligned" in L.wp_last_error()
    assert _device(v, _spec(), off=516)[0] == ARG and b"row_off must be 8-byte aligned" in L.wp_last_error()
    assert v.dedup_stats()["n_rows"] == -1  # none of these was a call


def test_bad_offsets_in_the_host_form_name_the_first_bad_row():
    L = W.lib()
    v = W.Vocab(VOCAB)
    data = b"abcdefgh"
    for off, row in (([1, 2, 3], 0), ([0, 3, 2, 8], 1), ([3, 2, 1], 0), ([0, 2, 4, 3], 2), ([0, 4, 2, 1], 1), ([-1, 2], 0), ([0, -1], 0)):
        for eb in (1, 4):
            rc, o = _host(v, data * 4, _off(off), _spec(elem_bytes=eb))
            assert rc == ARG and (b"row_off" in L.wp_last_error()) and L.wp_last_error().endswith(b"row %d" % row) and _cleared(o), (off, L.wp_last_error())
    # the Python mirror's own rules: offsets behind the data, a shape that is no row_off, data that is neither text nor ids
    with pytest.raises(W.WordPieceError, match="behind the data"):
        v.dedup_rows(b"abc", [0, 2, 4])
    with pytest.raises(W.WordPieceError, match="behind the data"):
        v.dedup_rows(np.zeros(3, dtype=np.int32), [0, 4])
    with pytest.raises(W.WordPieceError, match="n_rows \\+ 1"):
        v.dedup_rows(b"abc", [])
    with pytest.raises(W.WordPieceError, match="text .* or a flat int32"):
        v.dedup_rows(np.zeros(3, dtype=np.int64), [0, 3])
    with pytest.raises(W.WordPieceError, match="row_off"):
        v.dedup_rows(b"abc", [0, 2, 1])
    assert v.dedup_stats()["n_rows"] == -1


def test_no_row_and_all_empty_rows_need_no_device():
    L = W.lib()
    v = W.Vocab(VOCAB)
    for eb in (1, 4):
        for want in range(4):
            for hash_bits in (0, 8):
                rc, o = _host(v, None, _off([0]), _spec(eb, want, hash_bits))
                assert rc == 0 and not (o.first or o.kept or o.counts or o.inverse or o.data) and (o.n_rows, o.n_unique, o.n_elems) == (0, 0, 0)
                assert bool(o.row_off) == bool(want & 2)
                if o.row_off:
                    assert C.cast(o.row_off, C.POINTER(C.c_int64))[0] == 0
                    L.wp_free(o.row_off)
                assert v.dedup_stats() == dict.fromkeys(STAT_FIELDS, 0)
                rc, o = _device(v, _spec(eb, want, hash_bits), n_rows=0, data=0, off=0)
                assert rc == 0 and _cleared(o) and v.dedup_stats() == dict.fromkeys(STAT_FIELDS, 0)
    for n in (1, 2, 70_000):
        for inverse in (False, True):
            for compact in (False, True):
                exp = DM.dedup_rows(b"", [0] * (n + 1))
                for data, kw in ((b"", {}), (np.zeros(0, dtype=np.int32), {}), (b"never read", dict(hash_bits=9))):
                    got = v.dedup_rows(data, [0] * (n + 1), inverse=inverse, compact=compact, **kw)
                    assert got["first"].dtype == np.int32 and got["first"].tolist() == exp["first"]
                    assert got["kept"].dtype == np.int32 and got["kept"].tolist() == [0]
                    assert got["counts"].dtype == np.int64 and got["counts"].tolist() == [n]
                    assert ("inverse" in got) == inverse and ("data" in got) == compact == ("row_off" in got)
                    if inverse:
                        assert got["inverse"].dtype == np.int32 and got["inverse"].tolist() == exp["inverse"]
                    if compact:
                        assert len(got["data"]) == 0 and got["row_off"].dtype == np.int64 and got["row_off"].tolist() == [0, 0]
                    st = v.dedup_stats()
                    assert {k: st[k] for k in exp["stats"]} == exp["stats"] and st["n_rounds"] == st["n_chunks"] == st["n_compared"] == 0
    # the Python forms on nothing
    r = v.dedup_rows(b"", inverse=True, compact=True)  # the lines of the empty text: no line
    assert r["first"].shape == (0,) and r["kept"].shape == (0,) and r["counts"].shape == (0,) and r["data"] == b"" and r["row_off"].tolist() == [0]
    assert v.dedup_docs([]) [0] == [] and v.dedup_docs([])[1].shape == (0,)
    text, off = W.line_rows(b"a\nb\n\na")
    assert text.tobytes() == b"a\nb\n\na\n" and off.tolist() == [0, 2, 4, 5, 7]
    assert W.line_rows(b"a\n")[1].tolist() == [0, 2] and W.line_rows(b"")[1].tolist() == [0]


def test_no_cpu_fallback():
    if W.lib().wp_device_count() > 0:
        pytest.skip("GPU present")
    v = W.Vocab(VOCAB)
    L = W.lib()
    for data, off in ((b"abab", [0, 2, 4]), (b"a", [0, 0, 1])):
        rc, o = _host(v, data, _off(off), _spec())
        assert rc == NO_DEVICE and b"no HIP device" in L.wp_last_error() and _cleared(o)
    assert _device(v, _spec())[0] == NO_DEVICE and b"no HIP device" in L.wp_last_error()
    with pytest.raises(W.WordPieceError, match="no HIP device"):
        v.dedup_rows(b"a\nb\na\n")
    with pytest.raises(W.WordPieceError, match="no HIP device"):
        v.dedup_docs(["a", "b", "a"])
