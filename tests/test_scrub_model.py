"""CPU checks of the scrub: tests/scrub_model.py against an independent regular-expression form of both patterns and on
fixed rows; the entry points without a device: every argument rule with its field, the batch without bytes, and the header
against the ctypes mirrors."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import scrub_model as M
import wordpiece_amd as W
from wordpiece_amd import scrub as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB, ARG, TOO_LARGE = ["[UNK]", "a", "b"], 6, 2
LABEL = rb"[A-Za-z0-9](?:[A-Za-z0-9\-]{0,61}[A-Za-z0-9])?"
EMAIL_RE = re.compile(rb"(?<![A-Za-z0-9._%+\-@])(?=[A-Za-z0-9._%+\-]{1,64}@)[._%+\-]*([A-Za-z0-9][A-Za-z0-9._%+\-]*@(?=[A-Za-z0-9.\-]{0,255}(?![A-Za-z0-9.\-]))"
                      rb"LABEL(?:\.LABEL)*\.[A-Za-z]{2,63}(?![A-Za-z0-9\-]))".replace(b"LABEL", LABEL))
OCTET = rb"(?:25[0-5]|2[0-4][0-9]|1[0-9][0-9]|[1-9]?[0-9])"
IPV4_RE = re.compile(rb"(?<![A-Za-z0-9_.\x80-\xff])(OCTET(?:\.OCTET){3})\.?(?![0-9.A-Za-z_\x80-\xff])".replace(b"OCTET", OCTET))
PIECES = [b"a", b"Zq", b"7", b"0", b".", b".", b"@", b"@", b"-", b"_", b"com", b"1.2.3.4", b"x@y.zz", b"300", b"01", b"\xc3\xa9", b" "]


def test_the_model_against_regular_expressions():
    rng = random.Random(28)
    found = [0, 0, 0]
    for _ in range(6000):
        row = b"".join(rng.choice(PIECES) for _ in range(rng.randrange(1, 14)))
        es, ips = M.emails(row), [(s, e) for s, e, _ in M.ipv4s(row)]
        assert es == [m.span(1) for m in EMAIL_RE.finditer(row)], row
        assert ips == [m.span(1) for m in IPV4_RE.finditer(row)], row
        assert all(a[1] <= b[0] for a, b in zip(es, es[1:])), row  # e-mails are disjoint
        for s, e in ips:  # an address meets an e-mail only from inside
            inside = [a <= s and e <= b for a, b in es if s < b and a < e]
            assert all(inside), row
            found[2] += len(inside)
        found[0] += len(es)
        found[1] += len(ips)
    assert all(found), found  # the pieces do produce e-mails, addresses and addresses inside e-mails


FIXED = [(b"a@b.com@c.org", [(0, 7, 0)]), (b"user@8.8.8.8", [(5, 12, 1)]), (b"1.2.3.4@example.com", [(0, 19, 0)]), (b"at 8.8.8.8. Next", [(3, 10, 1)]),
         (b"v1.2.3.4", []), (b"10.0.0.1-10.0.0.5", [(0, 8, 2), (9, 17, 2)]), (b"x@example.com2", []), (b"foo@bar.com.", [(0, 11, 0)]),
         (b"..+me@a-b.xy.org-x", [(3, 12, 0)]), (b"a@b.c0m.net.x", [(0, 11, 0)]), (b"1.2.3.256 01.2.3.4 1.2.3 1.2.3.4.5 224.0.0.1", [(35, 44, 2)])]


@pytest.mark.parametrize("row,want", FIXED, ids=[r.decode() for r, _ in FIXED])
def test_fixed_rows(row, want):
    assert M.matches(row, M.EMAIL | M.IPV4 | M.KEEP_PRIVATE) == want
    assert M.fnv1a(b"A@b.Cc") == M.fnv1a(b"a@b.cc") == 0xF717CBE2 and M.fnv1a(b"") == 2166136261


def test_symbols_and_structs_match_the_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd_scrub.h")).read()
    assert sorted(re.findall(r"\b(wp_\w+)\s*\(", hdr.split("#ifndef")[1])) == sorted(S.ABI_SYMBOLS)
    assert all(hasattr(S.lib(), name) and name not in W.ABI_SYMBOLS for name in S.ABI_SYMBOLS)
    for prefix, names in (("WP_SS_BYTES = 0", S.SCRUB_SIGNALS), ("WP_SR_MAX_EMAILS = 0", S.SCRUB_RULES)):
        enum = re.search(r"enum \{ %s.*?\};" % prefix, hdr, re.S).group(0)
        assert [x.lower() for x in re.findall(r"WP_S[SR]_(\w+)", enum)] == list(names)
    assert (S.SCRUB_SIGNALS, S.SCRUB_RULES) == (M.SIGNALS, M.RULES)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd_scrub.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(wp_scrub_spec), offsetof(wp_scrub_spec, n_email_repl), offsetof(wp_scrub_spec, reserved),\n'
                   '         sizeof(wp_scrub_result), offsetof(wp_scrub_result, kept), offsetof(wp_scrub_result, n_elems), sizeof(wp_scrub_stats),\n'
                   '         offsetof(wp_scrub_stats, rule_failed), WP_SCRUB_SIGNALS, WP_SCRUB_WANT_MATCHES | WP_SCRUB_WANT_TEXT | WP_SCRUB_WANT_COMPACT,\n'
                   '         WP_SCRUB_EMAIL | WP_SCRUB_IPV4 | WP_SCRUB_IP_KEEP_PRIVATE);\n  return 0;\n}\n')
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "sz"), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "sz")], check=True, capture_output=True, text=True).stdout.split()]
    P, T, U = S.ScrubSpec, S.ScrubResult, S.ScrubStats
    assert got == [C.sizeof(P), P.n_email_repl.offset, P.reserved.offset, C.sizeof(T), T.kept.offset, T.n_elems.offset, C.sizeof(U), U.rule_failed.offset,
                   len(S.SCRUB_SIGNALS), 7, 7]
    assert (C.sizeof(P), C.sizeof(T), C.sizeof(U)) == (64, 136, 72)


def _spec(strings=(b"e", b"i"), n_email=1, off=None, **fields):
    """-> (ScrubSpec, what its pointers name)"""
    pool = np.frombuffer(b"".join(strings) + b"\0", dtype=np.uint8)
    off = np.asarray(np.cumsum([0] + [len(p) for p in strings]) if off is None else off, dtype=np.int64)
    s = S.ScrubSpec(1, 0, 3, 0, (C.c_int64 * 2)(-1, -1), n_email, len(strings) - n_email, pool.ctypes.data, off.ctypes.data, 0)
    for name, x in fields.items():
        if isinstance(x, tuple):
            getattr(s, name)[x[0]] = x[1]
        else:
            setattr(s, name, x)
    return s, (pool, off)


def _call(v, spec, data=b"abab", off=(0, 2, 4), out=True, n_rows=None, device=False):
    o = S.ScrubResult(*range(1, 18))  # (garbage in: the call clears it)
    off = None if off is None else np.asarray(off, dtype=np.int64)
    n = (0 if off is None else len(off) - 1) if n_rows is None else n_rows
    sp, op = None if spec is None else C.byref(spec), C.byref(o) if out else None
    if device:  # (pointers that are never dereferenced: the argument rules come first)
        return S.lib().wp_scrub_rows_device(v._h, C.c_void_p(data), None if off is None else C.c_void_p(512), n, sp, op), o
    return S.lib().wp_scrub_rows(v._h, data, None if off is None else off.ctypes.data, n, sp, op), o


BAD_SPECS = [
    (dict(elem_bytes=4), b"elem_bytes must be 1"), (dict(want=8), b"want"), (dict(kinds=8), b"kinds has bits outside 7"), (dict(pad=1), b"pad must be 0"),
    (dict(doc_limit=(0, -2)), b"doc_limit[0] must be -1 or in [0, 10^9]"), (dict(doc_limit=(1, 10 ** 9 + 1)), b"doc_limit[1]"),
    (dict(n_email_repl=17), b"n_email_repl must be in [0, 16]"), (dict(n_ip_repl=-1), b"n_ip_repl must be in [0, 16]"),
    (dict(n_email_repl=0), b"n_email_repl must be 1 at least"), (dict(n_ip_repl=0), b"n_ip_repl must be 1 at least"), (dict(repl_pool=None), b"repl_pool is NULL"),
    (dict(repl_off=None), b"repl_off is NULL"), (dict(off=[1, 2, 3]), b"repl_off must start at 0"), (dict(strings=[b"e", b"i" * 65]), b"string 1 must have 0 to 64 bytes"),
    (dict(off=[0, 2, 1]), b"string 1 must have 0 to 64 bytes"), (dict(strings=[b"e", b"a\nb"]), b"string 1 holds a line feed"), (dict(reserved=1), b"reserved must be 0"),
]


@pytest.mark.parametrize("fields,msg", BAD_SPECS, ids=[m.decode() for _, m in BAD_SPECS])
def test_argument_errors_come_before_the_device_and_name_the_field(fields, msg):
    v = W.Vocab(VOCAB)
    spec, hold = _spec(**fields)
    for how in (dict(), dict(data=b"", off=(0,)), dict(data=b"", off=(0, 0)), dict(device=True, data=256), dict(device=True, data=256, n_rows=0)):
        rc, o = _call(v, spec, **how)
        err = S.lib().wp_last_error()
        assert rc == ARG and msg in err and err.startswith(b"scrub: ") and not any(getattr(o, k) for k, _ in o._fields_), (how, err)
    assert S.scrub_stats(v)["n_rows"] == -1  # none of these was a call


def test_batch_errors_and_the_wrapper():
    v, last = W.Vocab(VOCAB), S.lib().wp_last_error
    plain, _ = _spec()
    assert _call(v, None)[0] == ARG and b"spec is NULL" in last()
    for device in (False, True):
        data = 256 if device else b"abab"
        assert _call(v, plain, data=data, out=False, device=device)[0] == ARG and b"out is NULL" in last()
        assert _call(v, plain, data=data, off=None, n_rows=2, device=device)[0] == ARG and b"row_off is NULL" in last()
        assert _call(v, plain, data=data, n_rows=2 ** 31, device=device)[0] == TOO_LARGE and b"2^31 rows or more in row_off" in last()
    assert _call(v, plain, data=None)[0] == ARG and b"scrub: data is NULL" in last()
    assert _call(v, plain, off=(0, 3, 2))[0] == ARG and last().endswith(b"row 1")
    assert _call(v, plain, off=(0, 2 ** 32))[0] == TOO_LARGE and b"UINT32_MAX" in last()
    assert S.scrub_stats(v)["n_rows"] == -1
    for text, how, match in ((np.zeros(3, dtype=np.int32), {}, "must be text"), (b"abc", dict(rules={"max_urls": 1}), "no such rule"), (b"abc", dict(kinds=["ipv6"]), "no such kind")):
        with pytest.raises(W.WordPieceError, match=match):
            S.scrub_rows(v, text, [0, 3], **how)
    assert S.scrub_replacements("default")["ip"] == ["192.0.2.1", "198.51.100.1", "203.0.113.1"] and "scrub_rows" not in dir(W)


@pytest.mark.parametrize("n", [0, 1, 3])
def test_a_batch_without_bytes_needs_no_device(n):
    v = W.Vocab(VOCAB)
    exp = M.scrub_rows(b"", [0] * (n + 1), rules={"max_emails": 0, "max_ips": 0})
    got = S.scrub_rows(v, b"", [0] * (n + 1), rules={"max_emails": 0, "max_ips": 0}, matches=True, text=True, compact=True)
    assert got["signals"].dtype == np.int64 and got["signals"].shape == (8, n) and got["reasons"].dtype == np.uint32 and got["reasons"].tolist() == [0] * n
    assert all(got[k].size == 0 for k in ("match_row", "match_start", "match_len", "match_kind", "match_repl")) and got["out_data"] == b"" == got["data"]
    assert got["out_off"].tolist() == exp["out_off"] and got["kept"].tolist() == exp["kept"] and got["row_off"].tolist() == exp["row_off"]
    assert S.scrub_stats(v) == exp["stats"] and sorted(S.scrub_rows(v, b"", [0] * (n + 1))) == ["reasons", "signals"]
    assert S.scrub_docs(v, [""] * n)[0] == [b""] * n and v.quality_stats()["n_rows"] == -1
