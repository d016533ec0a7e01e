"""CPU checks of the repetition entry points: header and exported symbols against the ctypes mirrors, every argument rule
with its field, the batch without bytes, the preset, and the model's own plausibility on the cases of the GPU test."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import repetition_cases as K
import repetition_model as M
import wordpiece_amd as W
from wordpiece_amd import repetition as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB, ARG, TOO_LARGE = ["[UNK]", "a", "b"], 6, 2


def test_symbols_and_structs_match_the_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd_repetition.h")).read()
    for name in R.ABI_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(R.lib(), name) and name not in W.ABI_SYMBOLS, name
    assert sorted(re.findall(r"\b(wp_\w+)\s*\(", hdr)) == sorted(R.ABI_SYMBOLS)
    enum = re.search(r"enum \{ WP_RPT_WORDS = 0,(.*?)\};", hdr, re.S).group(0)
    assert [x.lower() for x in re.findall(r"WP_RPT_(\w+)", enum)] == list(R.REPETITION_SIGNALS) == list(M.SIGNALS)
    assert R.REPETITION_RULES == M.RULES and re.search(r"#define WP_RPT_WANT_COMPACT\s+1\b", hdr) and R.WP_RPT_WANT_COMPACT == 1
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd_repetition.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(wp_stats), sizeof(wp_repetition_spec), offsetof(wp_repetition_spec, limit),\n'
                   '         offsetof(wp_repetition_spec, reserved), sizeof(wp_repetition_result), offsetof(wp_repetition_result, reasons),\n'
                   '         offsetof(wp_repetition_result, n_elems), sizeof(wp_repetition_stats), offsetof(wp_repetition_stats, rule_failed),\n'
                   '         WP_RPT_SIGNALS, WP_RPT_RULES);\n  return 0;\n}\n')
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "sz"), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "sz")], check=True, capture_output=True, text=True).stdout.split()]
    S, T, U = R.RepetitionSpec, R.RepetitionResult, R.RepetitionStats
    assert got == [C.sizeof(W.Stats), C.sizeof(S), S.limit.offset, S.reserved.offset, C.sizeof(T), T.reasons.offset, T.n_elems.offset, C.sizeof(U),
                   U.rule_failed.offset, len(R.REPETITION_SIGNALS), len(R.REPETITION_RULES)]
    assert (C.sizeof(S), C.sizeof(T), C.sizeof(U), got[-2:]) == (88, 64, 112, [14, 9])


def _spec(elem_bytes=1, want=0, limit=None, reserved=0):
    lim = [-1] * 9
    for k, value in (limit or {}).items():
        lim[k] = value
    return R.RepetitionSpec(elem_bytes, want, (C.c_int64 * 9)(*lim), reserved)


def _host(v, data, off, spec, out=True, n_rows=None):
    o = R.RepetitionResult(*range(1, 9))  # (garbage in: the call clears it)
    n = (len(off) - 1 if off is not None else 0) if n_rows is None else n_rows
    rc = R.lib().wp_repetition_rows(v._h, data, None if off is None else off.ctypes.data, n, None if spec is None else C.byref(spec), C.byref(o) if out else None)
    return rc, o


def _device(v, spec, n_rows=3, out=True, data=256, off=512):
    o = R.RepetitionResult(*range(1, 9))  # (pointers that are never dereferenced: the argument rules come first)
    rc = R.lib().wp_repetition_rows_device(v._h, C.c_void_p(data), None if off is None else C.c_void_p(off), n_rows, None if spec is None else C.byref(spec),
                                           C.byref(o) if out else None)
    return rc, o


_cleared = lambda o: not any(getattr(o, k) for k, _ in o._fields_)  # noqa: E731
_off = lambda values: np.array(values, dtype=np.int64)  # noqa: E731


def test_argument_errors_come_before_the_device_and_name_the_field():
    L = R.lib()
    v = W.Vocab(VOCAB)
    assert R.repetition_stats(v)["n_rows"] == -1
    cases = [(None, b"spec is NULL"), (_spec(elem_bytes=0), b"elem_bytes must be 1"), (_spec(elem_bytes=4), b"elem_bytes must be 1"), (_spec(want=2), b"want"),
             (_spec(want=-1), b"want"), (_spec(limit={0: -2}), b"limit[0] must be -1 or in [0, 1000]"), (_spec(limit={8: 1001}), b"limit[8]"),
             (_spec(limit={4: 2 ** 40}), b"limit[4]"), (_spec(reserved=1), b"reserved must be 0")]
    for spec, msg in cases:
        for data, off in ((b"abab", _off([0, 2, 4])), (b"", _off([0])), (b"", _off([0, 0]))):
            rc, o = _host(v, data, off, spec)
            assert rc == ARG and msg in L.wp_last_error() and L.wp_last_error().startswith(b"repetition: ") and _cleared(o), (msg, L.wp_last_error())
        for n_rows in (3, 0):
            rc, o = _device(v, spec, n_rows=n_rows)
            assert rc == ARG and msg in L.wp_last_error() and _cleared(o), (msg, L.wp_last_error())
    ab, o2, plain = b"abab", _off([0, 2, 4]), _spec()
    for call in (lambda: _host(v, ab, o2, plain, out=False), lambda: _device(v, plain, out=False)):
        assert call()[0] == ARG and b"out is NULL" in L.wp_last_error()
    assert _host(v, ab, None, plain, n_rows=2)[0] == ARG and b"row_off is NULL" in L.wp_last_error()
    assert _device(v, plain, off=None)[0] == ARG and b"row_off is NULL" in L.wp_last_error()
    assert _host(v, None, o2, plain)[0] == ARG and b"repetition: data is NULL" in L.wp_last_error()
    assert _host(v, ab, _off([0, 3, 2]), plain)[0] == ARG and L.wp_last_error().endswith(b"row 1")
    assert _host(v, ab, o2, plain, n_rows=2 ** 31)[0] == TOO_LARGE and b"2^31 rows or more in row_off" in L.wp_last_error()
    assert _host(v, ab, _off([0, 2 ** 32]), plain)[0] == TOO_LARGE and b"UINT32_MAX" in L.wp_last_error()
    assert _device(v, plain, data=257)[0] == ARG and b"repetition: data must be 4-byte aligned" in L.wp_last_error()
    assert R.repetition_stats(v)["n_rows"] == -1  # none of these was a call
    for text, match in ((np.zeros(3, dtype=np.int32), "must be text"), (b"abc", "no such rule")):
        with pytest.raises(W.WordPieceError, match=match):
            R.repetition_rows(v, text, [0, 3], rules={"max_top_5_chars": 1})
    with pytest.raises(W.WordPieceError, match="no such preset"):
        R.repetition_rules("c4")


def test_a_batch_without_bytes_needs_no_device():
    v = W.Vocab(VOCAB)
    assert M.limits(**R.repetition_rules("gopher")) == [200, 180, 160, 150, 140, 130, 120, 110, 100] == M.limits(**M.GOPHER)
    for n in (0, 1, 3):
        for rules in (None, "gopher", {"max_top_2_chars": 0, "max_dup_10_chars": 1000}):
            limit = M.limits(**(R.repetition_rules(rules) if isinstance(rules, str) else rules or {}))
            exp = M.repetition(b"", [0] * (n + 1), limit=limit)
            got = R.repetition_rows(v, b"", [0] * (n + 1), rules=rules, compact=True)
            assert got["signals"].dtype == np.int64 and got["signals"].shape == (14, n) and not got["signals"].any()
            assert got["reasons"].dtype == np.uint32 and got["reasons"].tolist() == exp["reasons"] == [0] * n
            assert got["kept"].tolist() == exp["kept"] and got["data"] == b"" and got["row_off"].tolist() == exp["row_off"]
            assert R.repetition_stats(v) == exp["stats"]
            assert sorted(R.repetition_rows(v, b"", [0] * (n + 1), rules=rules)) == ["reasons", "signals"]
    assert R.repetition_docs(v, ["", b""], rules="gopher")[0] == ["", b""] and v.quality_stats()["n_rows"] == -1


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_the_model_is_plausible(name):
    for row in K.CASES[name]():
        s = M.signals_of_row(row)
        for n in (2, 3, 4):
            count, chars = s[M.S["top_%d_count" % n]], s[M.S["top_%d_chars" % n]]
            assert (count >= 2 and chars >= count * n and chars % count == 0) or (count, chars) == (0, 0)
        dup = s[M.S["dup_5_chars"]:]
        assert all(0 <= d <= s[M.S["word_chars"]] for d in dup) and s[M.S["words"]] <= s[M.S["word_chars"]]
        assert s[M.S["words"]] < 10 or all(a >= b for a, b in zip(dup, dup[1:]))
