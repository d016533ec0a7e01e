"""CPU checks of the line-filter entry points: header and exported symbols against the ctypes mirrors, every argument rule
with its field, the call without rows and the batch without bytes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lines_model as M
import wordpiece_amd as W
from wordpiece_amd import lines as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB, ARG, TOO_LARGE = ["[UNK]", "a", "b"], 6, 2


def test_symbols_and_structs_match_the_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd_lines.h")).read()
    assert sorted(re.findall(r"\b(wp_\w+)\s*\(", hdr.split("#ifndef")[1])) == sorted(L.ABI_SYMBOLS)
    assert all(hasattr(L.lib(), name) and name not in W.ABI_SYMBOLS for name in L.ABI_SYMBOLS)
    for prefix, names in (("WP_LF_BYTES = 0", L.LINES_SIGNALS), ("WP_LR_MIN_WORDS = 0", L.LINE_RULES), ("WP_LD_MIN_KEPT_LINES = 0", L.DOC_RULES)):
        enum = re.search(r"enum \{ %s.*?\};" % prefix, hdr, re.S).group(0)
        assert [x.lower() for x in re.findall(r"WP_L[FRD]_(\w+)", enum)] == list(names)
    assert (L.LINES_SIGNALS, L.LINE_RULES, L.DOC_RULES) == (M.SIGNALS, M.LINE_RULES, M.DOC_RULES)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd_lines.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(wp_lines_spec), offsetof(wp_lines_spec, dup_scope), offsetof(wp_lines_spec, reserved),\n'
                   '         sizeof(wp_lines_result), offsetof(wp_lines_result, kept), offsetof(wp_lines_result, n_elems), sizeof(wp_lines_stats),\n'
                   '         offsetof(wp_lines_stats, rule_failed), WP_LF_SIGNALS, WP_LF_WANT_LINES | WP_LF_WANT_CUT | WP_LF_WANT_COMPACT,\n'
                   '         WP_LF_PHRASE_BOUNDED | WP_LF_PHRASE_DOC);\n  return 0;\n}\n')
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "sz"), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "sz")], check=True, capture_output=True, text=True).stdout.split()]
    S, T, U = L.LinesSpec, L.LinesResult, L.LinesStats
    assert got == [C.sizeof(S), S.dup_scope.offset, S.reserved.offset, C.sizeof(T), T.kept.offset, T.n_elems.offset, C.sizeof(U), U.rule_failed.offset,
                   len(L.LINES_SIGNALS), 7, 3]
    assert (C.sizeof(S), C.sizeof(T), C.sizeof(U)) == (120, 128, 136)


def _spec(phrases=(), flags=None, off=None, **fields):
    """-> (LinesSpec, what its pointers name)"""
    pool = np.frombuffer(b"".join(phrases) + b"\0", dtype=np.uint8)
    off = np.asarray(np.cumsum([0] + [len(p) for p in phrases]) if off is None else off, dtype=np.int64)
    flags = np.asarray([0] * len(phrases) if flags is None else flags, dtype=np.int32)
    s = L.LinesSpec(1, 0, (C.c_int64 * 4)(-1, -1, -1, -1), (C.c_int64 * 4)(-1, -1, -1, -1), 0, 0, len(phrases), 0, pool.ctypes.data, off.ctypes.data, flags.ctypes.data, 0)
    for name, x in fields.items():
        if isinstance(x, tuple):
            getattr(s, name)[x[0]] = x[1]
        else:
            setattr(s, name, x)
    return s, (pool, off, flags)


def _call(v, spec, data=b"abab", off=(0, 2, 4), out=True, n_rows=None, device=False):
    o = L.LinesResult(*range(1, 17))  # (garbage in: the call clears it)
    off = None if off is None else np.asarray(off, dtype=np.int64)
    n = (0 if off is None else len(off) - 1) if n_rows is None else n_rows
    sp, op = None if spec is None else C.byref(spec), C.byref(o) if out else None
    if device:  # (pointers that are never dereferenced: the argument rules come first)
        return L.lib().wp_filter_lines_device(v._h, C.c_void_p(data), None if off is None else C.c_void_p(512), n, sp, op), o
    return L.lib().wp_filter_lines(v._h, data, None if off is None else off.ctypes.data, n, sp, op), o


_cleared = lambda o: not any(getattr(o, k) for k, _ in o._fields_)  # noqa: E731
BAD_SPECS = [
    (dict(elem_bytes=4), b"elem_bytes must be 1"), (dict(want=8), b"want"), (dict(line_limit=(0, -2)), b"line_limit[0] must be -1 or in [0, 10^9]"),
    (dict(line_limit=(1, 10 ** 9 + 1)), b"line_limit[1]"), (dict(line_limit=(2, 1)), b"line_limit[2] must be 0 or -1"), (dict(line_limit=(3, 5)), b"line_limit[3] must be 0 or -1"),
    (dict(doc_limit=(0, -3)), b"doc_limit[0]"), (dict(doc_limit=(3, 2 ** 40)), b"doc_limit[3]"), (dict(dup_scope=3), b"dup_scope must be 0, 1 or 2"),
    (dict(dup_scope=-1), b"dup_scope"), (dict(dup_min_chars=-1), b"dup_min_chars must not be negative"), (dict(n_phrases=-1), b"n_phrases must be in [0, 512]"),
    (dict(n_phrases=513), b"n_phrases"), (dict(pad=1), b"pad must be 0"), (dict(reserved=1), b"reserved must be 0"),
    (dict(phrases=[b"a"], phrase_pool=None), b"phrase_pool is NULL"), (dict(phrases=[b"a"], phrase_off=None), b"phrase_off is NULL"),
    (dict(phrases=[b"a"], phrase_flags=None), b"phrase_flags is NULL"), (dict(phrases=[b"a"], off=[1, 2]), b"phrase_off must start at 0"),
    (dict(phrases=[b"a", b""]), b"phrase 1 must have 1 to 32 bytes"), (dict(phrases=[b"a" * 33]), b"phrase 0 must have 1 to 32 bytes"),
    (dict(phrases=[b"ok", b"xAy", b"B"]), b"phrase 1 holds ASCII upper case"), (dict(phrases=[b"a\nb"]), b"phrase 0 holds a line feed"),
    (dict(phrases=[b"a", b"b"], flags=[3, 4]), b"phrase 1 has bits outside 3"), (dict(phrases=[b"p" * 32] * 257), b"phrase 256 ends behind the 8192 bytes"),
]


@pytest.mark.parametrize("fields,msg", BAD_SPECS, ids=[m.decode() for _, m in BAD_SPECS])
def test_argument_errors_come_before_the_device_and_name_the_field(fields, msg):
    v = W.Vocab(VOCAB)
    spec, hold = _spec(**fields)
    for how in (dict(), dict(data=b"", off=(0,)), dict(data=b"", off=(0, 0)), dict(device=True, data=256), dict(device=True, data=256, n_rows=0)):
        rc, o = _call(v, spec, **how)
        err = L.lib().wp_last_error()
        assert rc == ARG and msg in err and err.startswith(b"lines: ") and _cleared(o), (how, err)
    assert L.lines_stats(v)["n_rows"] == -1  # none of these was a call


def test_batch_errors_and_the_wrapper():
    v, last = W.Vocab(VOCAB), L.lib().wp_last_error
    plain, _ = _spec()
    assert _call(v, None)[0] == ARG and b"spec is NULL" in last()
    for device in (False, True):
        data = 256 if device else b"abab"
        assert _call(v, plain, data=data, out=False, device=device)[0] == ARG and b"out is NULL" in last()
        assert _call(v, plain, data=data, off=None, n_rows=2, device=device)[0] == ARG and b"row_off is NULL" in last()
        assert _call(v, plain, data=data, n_rows=2 ** 31, device=device)[0] == TOO_LARGE and b"2^31 rows or more in row_off" in last()
    assert _call(v, plain, data=None)[0] == ARG and b"lines: data is NULL" in last()
    assert _call(v, plain, off=(0, 3, 2))[0] == ARG and last().endswith(b"row 1")
    assert _call(v, plain, off=(0, 2 ** 32))[0] == TOO_LARGE and b"UINT32_MAX" in last()
    assert _call(v, plain, data=257, device=True)[0] == ARG and b"lines: data must be 4-byte aligned" in last()
    assert L.lines_stats(v)["n_rows"] == -1
    for text, how, match in ((np.zeros(3, dtype=np.int32), {}, "must be text"), (b"abc", dict(rules={"min_lines": 1}), "no such rule"), (b"abc", dict(rules="c5"), "no such preset")):
        with pytest.raises(W.WordPieceError, match=match):
            L.filter_lines(v, text, [0, 3], **how)
    c4 = L.lines_rules("c4")
    assert len(c4["phrases"]) + len(c4["doc_phrases"]) == 9 and c4["rules"] == {"min_words": 3, "not_terminal": 0, "min_kept_lines": 5, "max_doc_phrase_hits": 0}


@pytest.mark.parametrize("n", [0, 1, 3])
@pytest.mark.parametrize("rules", [None, "c4", {"min_kept_words": 0, "max_dropped_x1000": 0, "max_doc_phrase_hits": 0}])
def test_a_batch_without_bytes_needs_no_device(n, rules):
    v = W.Vocab(VOCAB)
    how = L.lines_rules(rules) if isinstance(rules, str) else dict(rules=rules)
    exp = M.filter_lines(b"", [0] * (n + 1), **how)
    got = L.filter_lines(v, b"", [0] * (n + 1), rules=rules, lines=True, cut=True, compact=True)
    assert got["signals"].dtype == np.int64 and got["signals"].shape == (15, n) and not got["signals"].any()
    assert got["reasons"].dtype == np.uint32 and got["reasons"].tolist() == exp["reasons"] == [1 if rules == "c4" else 0] * n
    assert all(got[k].size == 0 for k in ("line_row", "line_start", "line_len", "line_reasons")) and got["cut_data"] == b"" == got["data"]
    assert got["cut_off"].tolist() == exp["cut_off"] and got["kept"].tolist() == exp["kept"] and got["row_off"].tolist() == exp["row_off"]
    assert L.lines_stats(v) == exp["stats"] and sorted(L.filter_lines(v, b"", [0] * (n + 1), rules=rules)) == ["reasons", "signals"]
    assert L.filter_docs(v, [""] * n, rules=rules)[0] == [b""] * len(exp["kept"]) and v.quality_stats()["n_rows"] == -1
