"""CPU checks of the quality entry points (wp_quality_rows, wp_quality_rows_device, wp_get_quality_stats): symbols and
structs against the header, what they answer without a device — every argument error with the field it names, the size
limits, bad offsets in the host form, no row, a batch without bytes, the statistics before any call — and that anything
else fails loudly without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import quality_model as M
import wordpiece_amd as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = ["[UNK]", "a", "b"]
ARG, TOO_LARGE, NO_DEVICE = 6, 2, 4
NAMES = ("wp_quality_rows", "wp_quality_rows_device", "wp_get_quality_stats", "wp_quality_class")
STAT_FIELDS = ["n_rows", "n_bytes", "n_chars", "n_invalid", "n_words", "n_lines", "n_dup_lines", "n_kept", "rule_failed"]
SPEC_FIELDS = ["elem_bytes", "want", "short_line_chars", "n_stop_words", "stop_pool", "stop_off", "limit", "reserved"]
RESULT_FIELDS = ["signals", "row_off", "reasons", "kept", "data", "n_rows", "n_kept", "n_elems"]
POINTERS = RESULT_FIELDS[:5]


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(W.LIB_PATH):
        from wordpiece_amd import build
        build.build()


def test_symbols_and_structs_match_the_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in W.ABI_SYMBOLS and hasattr(W.lib(), name), name
    assert "typedef struct { int32_t elem_bytes, want, short_line_chars, n_stop_words; const void *stop_pool; const int64_t *stop_off; " \
           "int64_t limit[WP_QUALITY_RULES]; int64_t reserved; } wp_quality_spec;" in hdr
    assert "typedef struct { int64_t *signals, *row_off; uint32_t *reasons; int32_t *kept; void *data; int64_t n_rows, n_kept, n_elems; } " \
           "wp_quality_result;" in hdr
    assert "typedef struct { int64_t n_rows, n_bytes, n_chars, n_invalid, n_words, n_lines, n_dup_lines, n_kept, rule_failed[WP_QUALITY_RULES]; } " \
           "wp_quality_stats;" in hdr
    for macro, value in (("WP_QUALITY_WANT_DUP_LINES", 1), ("WP_QUALITY_WANT_COMPACT", 2)):
        assert re.search(r"#define %s\s+%d\b" % (macro, value), hdr) and getattr(W, macro) == value
    assert re.search(r"#define WP_QUALITY_SIGNALS\s+23\b", hdr) and len(W.QUALITY_SIGNALS) == 23 and W.QUALITY_SIGNALS == M.SIGNALS
    assert re.search(r"#define WP_QUALITY_RULES\s+16\b", hdr) and len(W.QUALITY_RULES) == 16 and W.QUALITY_RULES == M.RULES
    # the names by index are the header's enumerators, in order
    qs = re.search(r"enum \{ WP_QS_BYTES = 0,(.*?)\};", hdr, re.S).group(0)
    assert [x.lower() for x in re.findall(r"WP_QS_(\w+)", qs)] == list(W.QUALITY_SIGNALS)
    qr = re.search(r"enum \{ WP_QR_MIN_TEXT_WORDS = 0,(.*?)\};", hdr, re.S).group(0)
    assert [x.lower() for x in re.findall(r"WP_QR_(\w+)", qr)] == list(W.QUALITY_RULES)
    assert [f[0] for f in W.QualitySpec._fields_] == SPEC_FIELDS
    assert [f[0] for f in W.QualityResult._fields_] == RESULT_FIELDS
    assert [f[0] for f in W.QualityStats._fields_] == STAT_FIELDS
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(wp_stats), sizeof(wp_quality_spec),\n'
                   '         offsetof(wp_quality_spec, stop_pool), offsetof(wp_quality_spec, limit), offsetof(wp_quality_spec, reserved),\n'
                   '         sizeof(wp_quality_result), offsetof(wp_quality_result, reasons), offsetof(wp_quality_result, data),\n'
                   '         offsetof(wp_quality_result, n_rows), offsetof(wp_quality_result, n_elems), sizeof(wp_quality_stats),\n'
                   '         offsetof(wp_quality_stats, rule_failed), sizeof(wp_repeat_stats), (int)WP_QS_DUP_LINE_CHARS, (int)WP_QR_RESERVED);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S, R, T = W.QualitySpec, W.QualityResult, W.QualityStats
    assert got == [C.sizeof(W.Stats), C.sizeof(S), S.stop_pool.offset, S.limit.offset, S.reserved.offset, C.sizeof(R), R.reasons.offset, R.data.offset,
                   R.n_rows.offset, R.n_elems.offset, C.sizeof(T), T.rule_failed.offset, C.sizeof(W.RepeatStats), 22, 15]
    assert C.sizeof(S) == 168 and C.sizeof(R) == 64 and C.sizeof(T) == 192
    assert [f[0] for f in W.Stats._fields_][-1] == "rows_route"  # wp_stats keeps its size and its end


def _spec(elem_bytes=1, want=0, short_line_chars=0, stop=None, limit=None, reserved=0, n_stop=None, pool=True, off=True, stop_off=None):
    """-> (spec, what it points into)"""
    words = [bytes(w) for w in (stop or ())]
    pool_arr = np.frombuffer(b"".join(words) + b"\0", dtype=np.uint8)
    off_arr = np.zeros(len(words) + 1, dtype=np.int64)
    if words:
        off_arr[1:] = np.cumsum([len(w) for w in words])
    if stop_off is not None:
        off_arr = np.array(stop_off, dtype=np.int64)
    lim = [-1] * 16
    for r, value in (limit or {}).items():
        lim[r] = value
    n = len(words) if n_stop is None else n_stop
    spec = W.QualitySpec(elem_bytes, want, short_line_chars, n, pool_arr.ctypes.data if pool else None, off_arr.ctypes.data if off else None,
                         (C.c_int64 * 16)(*lim), reserved)
    return spec, (pool_arr, off_arr)


def _off(values):
    return np.array(values, dtype=np.int64)


def _garbage():
    return W.QualityResult(*range(1, 9))  # (garbage in: the call clears it)


def _host(v, data, off, spec, out=True, n_rows=None):
    o = _garbage()
    n = (len(off) - 1 if off is not None else 0) if n_rows is None else n_rows
    rc = W.lib().wp_quality_rows(v._h, data, None if off is None else off.ctypes.data, n, None if spec is None else C.byref(spec), C.byref(o) if out else None)
    return rc, o


def _device(v, spec, n_rows=3, out=True, data=256, off=512):
    """the device form with pointers that are never dereferenced: the argument rules come first"""
    o = _garbage()
    rc = W.lib().wp_quality_rows_device(v._h, C.c_void_p(data), None if off is None else C.c_void_p(off), n_rows, None if spec is None else C.byref(spec),
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
    assert v.quality_stats()["n_rows"] == -1  # a fresh handle: no such call yet
    cases = [(None, b"spec is NULL"), (_spec(elem_bytes=0), b"elem_bytes"), (_spec(elem_bytes=4), b"elem_bytes"), (_spec(elem_bytes=2), b"elem_bytes"),
             (_spec(want=4), b"want"), (_spec(want=-1), b"want"), (_spec(short_line_chars=-1), b"short_line_chars"),
             (_spec(limit={0: -2}), b"limit[0]"), (_spec(limit={3: 10 ** 9 + 1}), b"limit[3]"), (_spec(limit={14: -(2 ** 40)}), b"limit[14]"),
             (_spec(limit={15: 0}), b"limit[15]"), (_spec(limit={15: 5}), b"limit[15] is reserved"),
             (_spec(limit={10: 300}), b"limit[10] needs WP_QUALITY_WANT_DUP_LINES"), (_spec(want=2, limit={11: 0}), b"limit[11] needs"),
             (_spec(n_stop=-1), b"n_stop_words"), (_spec(n_stop=65), b"n_stop_words"), (_spec(stop=[b"the"], pool=False), b"stop_pool is NULL"),
             (_spec(stop=[b"the"], off=False), b"stop_off is NULL"), (_spec(stop=[b"the"], stop_off=[1, 3]), b"stop_off must start at 0"),
             (_spec(stop=[b"the", b"of"], stop_off=[0, 3, 3]), b"stop_off: word 1"), (_spec(stop=[b"the", b"of"], stop_off=[0, 3, 2]), b"stop_off: word 1"),
             (_spec(stop=[b"x" * 33]), b"stop_off: word 0"), (_spec(stop=[b"ok", b"The"]), b"stop_pool: word 1 holds ASCII upper case"),
             (_spec(reserved=1), b"reserved"), (_spec(reserved=-1), b"reserved")]
    for spec, msg in cases:
        spec, keep = spec if spec is not None else (None, None)
        for data, off in ((b"abab", _off([0, 2, 4])), (b"", _off([0])), (b"", _off([0, 0]))):
            rc, o = _host(v, data, off, spec)
            assert rc == ARG and msg in L.wp_last_error() and L.wp_last_error().startswith(b"quality: ") and _cleared(o), (msg, L.wp_last_error())
        for n_rows in (3, 0):
            rc, o = _device(v, spec, n_rows=n_rows)
            assert rc == ARG and msg in L.wp_last_error() and _cleared(o), (msg, L.wp_last_error())
    ab, o2 = b"abab", _off([0, 2, 4])
    plain, keep = _spec()
    for call in (lambda: _host(v, ab, o2, plain, out=False), lambda: _device(v, plain, out=False)):
        assert call()[0] == ARG and b"out is NULL" in L.wp_last_error()
    assert _host(v, ab, None, plain, n_rows=2)[0] == ARG and b"row_off is NULL" in L.wp_last_error()
    assert _device(v, plain, off=None)[0] == ARG and b"row_off is NULL" in L.wp_last_error()
    assert _host(v, None, o2, plain)[0] == ARG and b"quality: data is NULL" in L.wp_last_error()
    assert _host(v, ab, o2, plain, n_rows=2 ** 31)[0] == TOO_LARGE and b"2^31 rows or more in row_off" in L.wp_last_error()
    assert _device(v, plain, n_rows=2 ** 31)[0] == TOO_LARGE and b"in row_off" in L.wp_last_error()
    assert _host(v, ab, _off([0, 2 ** 32]), plain)[0] == TOO_LARGE and b"UINT32_MAX" in L.wp_last_error()
    assert _device(v, plain, data=257)[0] == ARG and b"quality: data must be 4-byte aligned" in L.wp_last_error()
    assert _device(v, plain, off=516)[0] == ARG and b"row_off must be 8-byte aligned" in L.wp_last_error()
    assert v.quality_stats()["n_rows"] == -1  # none of these was a call
    # the limits at their ends, a full stop list and words of 32 bytes are fine
    ok, keep = _spec(want=3, limit={r: 10 ** 9 for r in range(15)}, stop=[bytes([97 + k % 26]) * (1 + k % 32) for k in range(64)])
    rc, o = _host(v, b"", _off([0, 0]), ok)
    assert rc == 0 and o.n_rows == 1
    _free(o)


def test_bad_offsets_in_the_host_form_name_the_first_bad_row():
    L = W.lib()
    v = W.Vocab(VOCAB)
    data = b"abcdefgh" * 4
    plain, keep = _spec()
    for off, row in (([1, 2, 3], 0), ([0, 3, 2, 8], 1), ([3, 2, 1], 0), ([0, 2, 4, 3], 2), ([0, 4, 2, 1], 1), ([-1, 2], 0), ([0, -1], 0)):
        rc, o = _host(v, data, _off(off), plain)
        err = L.wp_last_error()
        assert rc == ARG and b"row_off" in err and err.endswith(b"row %d" % row) and _cleared(o), (off, err)
    # the Python mirror's own rules
    with pytest.raises(W.WordPieceError, match="ends behind the data"):
        v.quality_rows(b"abc", [0, 2, 4])
    with pytest.raises(W.WordPieceError, match="n_rows \\+ 1"):
        v.quality_rows(b"abc", [])
    with pytest.raises(W.WordPieceError, match="must be text"):
        v.quality_rows(np.zeros(3, dtype=np.int32), [0, 3])
    with pytest.raises(W.WordPieceError, match="row_off"):
        v.quality_rows(b"abc", [0, 2, 1])
    with pytest.raises(W.WordPieceError, match="no such rule"):
        v.quality_rows(b"", [0, 0], rules={"max_words": 3})
    with pytest.raises(W.WordPieceError, match="no such rule"):
        v.quality_rows(b"", [0, 0], rules={"reserved": 3})
    with pytest.raises(W.WordPieceError, match="no such preset"):
        W.quality_rules("c4")
    with pytest.raises(W.WordPieceError, match="upper case"):
        v.quality_rows(b"", [0, 0], stop_words=["The"])
    with pytest.raises(W.WordPieceError, match=r"limit\[10\] needs"):
        v.quality_rows(b"", [0, 0], rules={"max_dup_lines": 300}, dup_lines=False)
    assert v.quality_stats()["n_rows"] == -1


def test_presets_are_the_models():
    for name in ("gopher", "fineweb"):
        rules = W.quality_rules(name)
        stop = tuple(w.encode() for w in rules.pop("stop_words", ()))
        assert M.limits(**rules) == M.PRESETS[name]["limit"] and stop == tuple(M.PRESETS[name]["stop_words"])
    assert W.quality_rules("gopher")["min_text_words"] == 50 and W.quality_rules("fineweb")["max_short_lines"] == 670


def test_no_row_needs_no_device():
    v = W.Vocab(VOCAB)
    for want in range(4):
        spec, keep = _spec(want=want, limit={0: 1})
        rc, o = _host(v, None, _off([0]), spec)
        assert rc == 0 and _cleared(o)
        st = v.quality_stats()
        assert all(st[k] == 0 for k in STAT_FIELDS[:-1]) and st["rule_failed"] == [0] * 16
        rc, o = _device(v, spec, n_rows=0, data=0, off=0)
        assert rc == 0 and _cleared(o)
    r = v.quality_rows(b"", None, rules={"min_text_words": 1}, compact=True)  # the lines of the empty text: no line
    assert r["signals"].shape == (23, 0) and r["reasons"].shape == (0,) and r["kept"].shape == (0,) and r["data"] == b"" and r["row_off"].tolist() == [0]
    assert v.quality_docs([])[0] == [] and v.quality_docs([])[1].shape == (0,)


def test_a_batch_without_bytes_needs_no_device():
    v = W.Vocab(VOCAB)
    for n in (1, 3):
        off = [0] * (n + 1)
        for rules in ({}, {"min_text_words": 1}, {"min_text_words": 0, "min_mean_word_x1000": 3000, "max_hash_per_word": 0, "min_alpha_words": 800,
                                                 "min_terminal_lines": 120, "max_dup_line_chars": 0}, {"min_stop_words": 2, "min_text_words": 50}):
            exp = M.quality(b"", off, limit=M.limits(**rules))
            got = v.quality_rows(b"", off, rules=rules, compact=True)
            assert got["signals"].dtype == np.int64 and got["signals"].tolist() == exp["signals"] and got["signals"].shape == (23, n)
            assert got["reasons"].dtype == np.uint32 and got["reasons"].tolist() == exp["reasons"]
            assert got["kept"].dtype == np.int32 and got["kept"].tolist() == exp["kept"] and got["data"] == b"" and got["row_off"].tolist() == exp["row_off"]
            assert v.quality_stats() == exp["stats"]
            plain = v.quality_rows(b"", off, rules=rules)
            assert sorted(plain) == ["reasons", "signals"]
    docs, reasons = v.quality_docs(["", b""], rules={"min_text_words": 1})
    assert docs == [] and reasons.tolist() == [1, 1]
    docs, reasons = v.quality_docs(["", b""])
    assert docs == ["", b""] and reasons.tolist() == [0, 0]
    other = W.Vocab(VOCAB)
    assert other.quality_stats()["n_rows"] == -1 and other.dedup_stats()["n_rows"] == -1


def test_no_cpu_fallback():
    if W.lib().wp_device_count() > 0:
        pytest.skip("GPU present")
    v = W.Vocab(VOCAB)
    L = W.lib()
    plain, keep = _spec()
    for data, off in ((b"abab", [0, 2, 4]), (b"ab", [0, 0, 2])):
        rc, o = _host(v, data, _off(off), plain)
        assert rc == NO_DEVICE and b"no HIP device" in L.wp_last_error() and _cleared(o)
    assert _device(v, plain)[0] == NO_DEVICE and b"no HIP device" in L.wp_last_error()
    with pytest.raises(W.WordPieceError, match="no HIP device"):
        v.quality_rows(b"ab\ncd\n", None)
    with pytest.raises(W.WordPieceError, match="no HIP device"):
        v.quality_docs(["abc", "bcd"], rules="gopher")
    assert v.quality_stats()["n_rows"] == -1
