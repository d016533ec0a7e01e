"""CPU checks of the neardup entry points (wp_neardup_rows, wp_neardup_rows_device, wp_get_neardup_stats): symbols and
structs against the header, what they answer without a device — every argument error with the field it names, the size
limits, bad offsets in the host form, no row, rows that are all empty, the statistics before any call — and that
anything else fails loudly without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import neardup_model as M
import wordpiece_amd as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = ["[UNK]", "a", "b"]
ARG, TOO_LARGE, NO_DEVICE = 6, 2, 4
NAMES = ("wp_neardup_rows", "wp_neardup_rows_device", "wp_get_neardup_stats")
STAT_FIELDS = ["n_rows", "n_unique", "n_empty", "n_elems", "n_shingles", "n_buckets", "n_candidates", "n_edges", "n_rounds"]
RESULT_FIELDS = ["cluster", "kept", "inverse", "counts", "row_off", "data", "signatures", "n_rows", "n_unique", "n_elems", "n_perm"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(W.LIB_PATH):
        from wordpiece_amd import build
        build.build()


def test_symbols_and_structs_match_the_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in W.ABI_SYMBOLS and hasattr(W.lib(), name), name
    assert re.search(r"typedef struct \{ int32_t elem_bytes, want, shingle, n_perm, bands, min_agree; uint64_t seed; int32_t reserved\[2\]; \} "
                     r"wp_neardup_spec;", hdr)
    assert re.search(r"typedef struct \{ int32_t \*cluster, \*kept, \*inverse; int64_t \*counts, \*row_off; void \*data; uint32_t \*signatures; "
                     r"int64_t n_rows, n_unique, n_elems, n_perm; \} wp_neardup_result;", hdr)
    assert re.search(r"typedef struct \{ int64_t %s; \} wp_neardup_stats;" % ", ".join(STAT_FIELDS), hdr)
    for macro, value in (("WP_NEARDUP_WANT_INVERSE", 1), ("WP_NEARDUP_WANT_COMPACT", 2), ("WP_NEARDUP_WANT_SIGNATURES", 4)):
        assert re.search(r"#define %s\s+%d\b" % (macro, value), hdr) and getattr(W, macro) == value
    assert re.search(r"#define WP_ERR_INTERNAL\s+7\b", hdr)
    assert [f[0] for f in W.NearDupSpec._fields_] == ["elem_bytes", "want", "shingle", "n_perm", "bands", "min_agree", "seed", "reserved"]
    assert [f[0] for f in W.NearDupResult._fields_] == RESULT_FIELDS
    assert [(n, C.sizeof(t)) for n, t in W.NearDupStats._fields_] == [(n, 8) for n in STAT_FIELDS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(wp_stats), sizeof(wp_neardup_spec),\n'
                   '         offsetof(wp_neardup_spec, min_agree), offsetof(wp_neardup_spec, seed), offsetof(wp_neardup_spec, reserved),\n'
                   '         sizeof(wp_neardup_result), offsetof(wp_neardup_result, counts), offsetof(wp_neardup_result, signatures),\n'
                   '         offsetof(wp_neardup_result, n_rows), offsetof(wp_neardup_result, n_perm), sizeof(wp_neardup_stats),\n'
                   '         offsetof(wp_neardup_stats, n_rounds), sizeof(wp_dedup_stats));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S, R = W.NearDupSpec, W.NearDupResult
    assert got == [C.sizeof(W.Stats), C.sizeof(S), S.min_agree.offset, S.seed.offset, S.reserved.offset, C.sizeof(R), R.counts.offset,
                   R.signatures.offset, R.n_rows.offset, R.n_perm.offset, C.sizeof(W.NearDupStats), W.NearDupStats.n_rounds.offset,
                   C.sizeof(W.DedupStats)]
    assert C.sizeof(S) == 40 and C.sizeof(R) == 88 and C.sizeof(W.NearDupStats) == 72
    assert [f[0] for f in W.Stats._fields_][-1] == "rows_route"  # wp_stats keeps its size and its end


def _spec(elem_bytes=1, want=0, shingle=5, n_perm=128, bands=16, min_agree=0, seed=0, reserved=(0, 0)):
    return W.NearDupSpec(elem_bytes, want, shingle, n_perm, bands, min_agree, seed, (C.c_int32 * 2)(*reserved))


def _off(values):
    return np.array(values, dtype=np.int64)


def _garbage():
    return W.NearDupResult(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)  # (garbage in: the call clears it)


def _host(v, data, off, spec, out=True, n_rows=None):
    o = _garbage()
    n = (len(off) - 1 if off is not None else 0) if n_rows is None else n_rows
    rc = W.lib().wp_neardup_rows(v._h, data, None if off is None else off.ctypes.data, n, None if spec is None else C.byref(spec),
                                 C.byref(o) if out else None)
    return rc, o


def _device(v, spec, n_rows=3, out=True, data=256, off=512):
    """the device form with pointers that are never dereferenced: the argument rules come first"""
    o = _garbage()
    rc = W.lib().wp_neardup_rows_device(v._h, C.c_void_p(data), None if off is None else C.c_void_p(off), n_rows,
                                        None if spec is None else C.byref(spec), C.byref(o) if out else None)
    return rc, o


def _cleared(o):
    return not (o.cluster or o.kept or o.inverse or o.counts or o.row_off or o.data or o.signatures) and \
        (o.n_rows, o.n_unique, o.n_elems, o.n_perm) == (0, 0, 0, 0)


def test_argument_errors_come_before_the_device_and_name_the_field():
    L = W.lib()
    v = W.Vocab(VOCAB)
    assert v.neardup_stats()["n_rows"] == -1  # a fresh handle: no such call yet
    cases = [(None, b"spec is NULL"), (_spec(elem_bytes=0), b"elem_bytes"), (_spec(elem_bytes=2), b"elem_bytes"), (_spec(elem_bytes=-4), b"elem_bytes"),
             (_spec(want=8), b"want"), (_spec(want=-1), b"want"), (_spec(shingle=0), b"shingle"), (_spec(shingle=65), b"shingle"),
             (_spec(shingle=-1), b"shingle"), (_spec(n_perm=0, bands=1), b"n_perm"), (_spec(n_perm=257, bands=1), b"n_perm"),
             (_spec(n_perm=-128), b"n_perm"), (_spec(bands=0), b"bands"), (_spec(bands=-1), b"bands"), (_spec(bands=3), b"bands"),
             (_spec(bands=256), b"bands"), (_spec(min_agree=-1), b"min_agree"), (_spec(min_agree=129), b"min_agree"),
             (_spec(reserved=(1, 0)), b"reserved"), (_spec(reserved=(0, 1)), b"reserved")]
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
    assert _device(v, _spec(n_perm=128, bands=1), n_rows=2 ** 25)[0] == TOO_LARGE and b"n_rows * n_perm" in L.wp_last_error()
    assert _device(v, _spec(n_perm=256, bands=256), n_rows=2 ** 24)[0] == TOO_LARGE and b"n_rows * n_perm" in L.wp_last_error()
    assert _host(v, b"a", _off([0, 1]), _spec(n_perm=4, bands=4), n_rows=2 ** 31 - 1)[0] == TOO_LARGE and b"n_rows * n_perm" in L.wp_last_error()
    assert _host(v, b"a", _off([0, 2 ** 32]), _spec())[0] == TOO_LARGE and b"UINT32_MAX" in L.wp_last_error()
    assert _host(v, b"a", _off([0, 2 ** 30]), _spec(elem_bytes=4))[0] == TOO_LARGE and b"UINT32_MAX" in L.wp_last_error()
    assert _device(v, _spec(), data=257)[0] == ARG and b"data must be 4-byte aligned" in L.wp_last_error()
    assert _device(v, _spec(), off=516)[0] == ARG and b"row_off must be 8-byte aligned" in L.wp_last_error()
    assert v.neardup_stats()["n_rows"] == -1  # none of these was a call


def test_bad_offsets_in_the_host_form_name_the_first_bad_row():
    L = W.lib()
    v = W.Vocab(VOCAB)
    data = b"abcdefgh"
    for off, row in (([1, 2, 3], 0), ([0, 3, 2, 8], 1), ([3, 2, 1], 0), ([0, 2, 4, 3], 2), ([0, 4, 2, 1], 1), ([-1, 2], 0), ([0, -1], 0)):
        for eb in (1, 4):
            rc, o = _host(v, data * 4, _off(off), _spec(elem_bytes=eb))
            assert rc == ARG and (b"row_off" in L.wp_last_error()) and L.wp_last_error().endswith(b"row %d" % row) and _cleared(o), (off, L.wp_last_error())
    # the Python mirror's own rules
    with pytest.raises(W.WordPieceError, match="behind the data"):
        v.neardup_rows(b"abc", [0, 2, 4])
    with pytest.raises(W.WordPieceError, match="n_rows \\+ 1"):
        v.neardup_rows(b"abc", [])
    with pytest.raises(W.WordPieceError, match="text .* or a flat int32"):
        v.neardup_rows(np.zeros(3, dtype=np.int64), [0, 3])
    with pytest.raises(W.WordPieceError, match="row_off"):
        v.neardup_rows(b"abc", [0, 2, 1])
    with pytest.raises(W.WordPieceError, match="bands"):
        v.neardup_rows(b"abc", [0, 3], n_perm=128, bands=5)
    assert v.neardup_stats()["n_rows"] == -1


def test_no_row_and_all_empty_rows_need_no_device():
    L = W.lib()
    v = W.Vocab(VOCAB)
    zero = dict.fromkeys(STAT_FIELDS, 0)
    for eb in (1, 4):
        for want in range(8):
            rc, o = _host(v, None, _off([0]), _spec(eb, want))
            assert rc == 0 and not (o.cluster or o.kept or o.counts or o.inverse or o.data or o.signatures)
            assert (o.n_rows, o.n_unique, o.n_elems, o.n_perm) == (0, 0, 0, 128) and bool(o.row_off) == bool(want & 2)
            if o.row_off:
                assert C.cast(o.row_off, C.POINTER(C.c_int64))[0] == 0
                L.wp_free(o.row_off)
            assert v.neardup_stats() == zero
            rc, o = _device(v, _spec(eb, want), n_rows=0, data=0, off=0)
            assert rc == 0 and _cleared(o) and v.neardup_stats() == zero
    for n in (1, 2, 70_000):
        exp = M.neardup_rows(b"", [0] * (n + 1), n_perm=4, bands=2)
        for inverse in (False, True):
            for compact in (False, True):
                for signatures in (False, True):
                    for data in (b"", np.zeros(0, dtype=np.int32), b"never read"):
                        got = v.neardup_rows(data, [0] * (n + 1), n_perm=4, bands=2, inverse=inverse, compact=compact, signatures=signatures)
                        assert got["cluster"].dtype == np.int32 and got["cluster"].tolist() == exp["cluster"] == list(range(n))
                        assert got["kept"].dtype == np.int32 and got["kept"].tolist() == exp["kept"]
                        assert got["counts"].dtype == np.int64 and got["counts"].tolist() == exp["counts"] == [1] * n
                        assert ("inverse" in got) == inverse and ("data" in got) == compact == ("row_off" in got) and ("signatures" in got) == signatures
                        if inverse:
                            assert got["inverse"].dtype == np.int32 and got["inverse"].tolist() == exp["inverse"]
                        if compact:
                            assert len(got["data"]) == 0 and got["row_off"].dtype == np.int64 and got["row_off"].tolist() == [0] * (n + 1)
                        if signatures:
                            assert got["signatures"].dtype == np.uint32 and got["signatures"].shape == (n, 4)
                            assert np.array_equal(got["signatures"], exp["signatures"]) and (got["signatures"] == 0xffffffff).all()
                        st = v.neardup_stats()
                        assert {k: st[k] for k in exp["stats"]} == exp["stats"] and st["n_rounds"] == 0 and st["n_unique"] == st["n_empty"] == n
    # the Python forms on nothing
    r = v.neardup_rows(b"", inverse=True, compact=True, signatures=True)  # the lines of the empty text: no line
    assert r["cluster"].shape == (0,) and r["kept"].shape == (0,) and r["counts"].shape == (0,) and r["data"] == b"" and r["row_off"].tolist() == [0]
    assert r["signatures"].shape == (0, 128)
    assert v.neardup_docs([])[0] == [] and v.neardup_docs([])[1].shape == (0,)


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
        v.neardup_rows(b"a\nb\na\n")
    with pytest.raises(W.WordPieceError, match="no HIP device"):
        v.neardup_docs(["a", "b", "a"])
