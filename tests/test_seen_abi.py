"""CPU checks of the seen-rows layer: the header against the ctypes mirrors and the library's exports, every argument rule
before a device is needed, the calls that need none, and the key of tests/seen_model.py at its chunk and length edges."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import seen_model as M
import wordpiece_amd as W
from wordpiece_amd import seen as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB, ARG, TOO_LARGE = ["[UNK]", "a", "b"], 6, 2


def test_symbols_and_structs_match_the_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd_seen.h")).read()
    assert sorted(re.findall(r"\b(wp_\w+)\s*\(", hdr.split("#ifndef")[1])) == sorted(S.ABI_SYMBOLS)
    assert all(hasattr(S.lib(), name) and name not in W.ABI_SYMBOLS for name in S.ABI_SYMBOLS) and "seen_rows" not in dir(W)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd_seen.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(wp_seen_spec), offsetof(wp_seen_spec, flags), offsetof(wp_seen_spec, reserved),\n'
                   '         sizeof(wp_seen_result), offsetof(wp_seen_result, keys), offsetof(wp_seen_result, n_kept), sizeof(wp_seen_stats),\n'
                   '         offsetof(wp_seen_stats, n_grown), WP_SEEN_WANT_KEYS | WP_SEEN_WANT_COMPACT, WP_SEEN_QUERY_ONLY, WP_SEEN_MIN_SLOTS, WP_SEEN_BEFORE);\n'
                   '  return 0;\n}\n')
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "sz"), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "sz")], check=True, capture_output=True, text=True).stdout.split()]
    P, T, U = S.SeenSpec, S.SeenResult, S.SeenStats
    assert got == [C.sizeof(P), P.flags.offset, P.reserved.offset, C.sizeof(T), T.keys.offset, T.n_kept.offset, C.sizeof(U), U.n_grown.offset,
                   S.WP_SEEN_WANT_KEYS | S.WP_SEEN_WANT_COMPACT, S.WP_SEEN_QUERY_ONLY, S.WP_SEEN_MIN_SLOTS, len(S.SEEN_STATES) - 1]
    assert (C.sizeof(P), C.sizeof(T), C.sizeof(U)) == (24, 72, 64)


def _call(v, spec, fn="rows", device=False, out=True, data=b"abab", off=(0, 2, 4), n=None):
    """one of the four calls with a result full of garbage (the call clears it) -> (code, result)"""
    o = S.SeenResult(*range(1, 10))
    sp, op = None if spec is None else C.byref(spec), C.byref(o) if out else None
    if fn == "keys":
        keys = np.arange(3, dtype=np.uint64)
        return getattr(S.lib(), "wp_seen_keys" + "_device" * device)(v._h, C.c_void_p(512) if device else keys.ctypes.data, 3 if n is None else n, sp, op), o
    off = None if off is None else np.asarray(off, dtype=np.int64)
    n = (0 if off is None else len(off) - 1) if n is None else n
    if device:  # (pointers that are never dereferenced: the argument rules come first)
        return S.lib().wp_seen_rows_device(v._h, C.c_void_p(256), None if off is None else C.c_void_p(512), n, sp, op), o
    return S.lib().wp_seen_rows(v._h, data, None if off is None else off.ctypes.data, n, sp, op), o


BAD_SPECS = [("rows", dict(elem_bytes=2), b"elem_bytes must be 1 or 4"), ("rows", dict(want=4), b"want has bits outside 3"), ("keys", dict(want=1), b"want must be 0"),
             ("rows", dict(flags=2), b"flags has bits outside 1"), ("keys", dict(flags=2), b"flags has bits outside 1"), ("rows", dict(pad=1), b"pad must be 0"),
             ("rows", dict(reserved=1), b"reserved must be 0"), ("keys", dict(reserved=-1), b"reserved must be 0")]


@pytest.mark.parametrize("fn,fields,msg", BAD_SPECS, ids=["%s: %s" % (f, m.decode()) for f, _, m in BAD_SPECS])
def test_argument_errors_come_before_the_device_and_name_the_field(fn, fields, msg):
    v = W.Vocab(VOCAB)
    spec = S.SeenSpec(1, 0, 0, 0, 0)
    for name, x in fields.items():
        setattr(spec, name, x)
    for device in (False, True):
        for n in (None, 0):
            rc, o = _call(v, spec, fn, device, n=n)
            err = S.lib().wp_last_error()
            assert rc == ARG and msg in err and err.startswith(b"seen: ") and not any(getattr(o, k) for k, _ in o._fields_), (device, n, err)
    assert S.seen_stats(v)["n_rows"] == -1  # none of these was a call


def test_batch_errors():
    v, last, plain = W.Vocab(VOCAB), S.lib().wp_last_error, S.SeenSpec(1, 0, 0, 0, 0)
    for fn in ("rows", "keys"):
        assert _call(v, None, fn)[0] == ARG and b"spec is NULL" in last()
        for device in (False, True):
            assert _call(v, plain, fn, device, out=False)[0] == ARG and b"out is NULL" in last()
            assert _call(v, plain, fn, device, n=2 ** 31)[0] == TOO_LARGE and b"2^31 rows or more" in last()
    for device in (False, True):
        assert _call(v, plain, device=device, off=None, n=2)[0] == ARG and b"row_off is NULL" in last()
    assert S.lib().wp_seen_keys(v._h, None, 2, C.byref(plain), C.byref(S.SeenResult())) == ARG and b"keys is NULL" in last()
    assert _call(v, plain, data=None)[0] == ARG and b"seen: data is NULL" in last()
    assert _call(v, plain, off=(0, 3, 2))[0] == ARG and last().endswith(b"row 1")  # descending offsets, host form
    assert _call(v, plain, off=(1, 2))[0] == ARG and last().endswith(b"row 0")
    assert _call(v, plain, off=(0, 2 ** 32))[0] == TOO_LARGE and b"UINT32_MAX" in last()
    assert S.lib().wp_seen_export(v._h, None, 4, C.byref(C.c_size_t())) == ARG and b"keys_out is NULL" in last()
    assert S.lib().wp_seen_export(v._h, None, 0, None) == ARG and b"n is NULL" in last()
    assert S.lib().wp_seen_reserve(v._h, 2 ** 31) == TOO_LARGE and b"2^31 slots" in last()
    assert S.seen_stats(v)["n_rows"] == -1
    with pytest.raises(W.WordPieceError, match="flat uint64"):
        S.seen_add_keys(v, np.zeros((2, 2), dtype=np.uint64))


def test_what_needs_no_device():
    v = W.Vocab(VOCAB)
    assert S.seen_stats(v) == dict(n_rows=-1, n_new=0, n_repeat_batch=0, n_seen_before=0, n_keys=0, capacity=0, n_grown=0, n_probes=0)
    got = S.seen_rows(v, b"", [0], keys=True, compact=True)
    assert [(k, x.dtype, len(x)) for k, x in got.items() if k != "data"] == [("state", np.int32, 0), ("first", np.int32, 0), ("keys", np.uint64, 0), ("kept", np.int32, 0),
                                                                            ("row_off", np.int64, 1)] and got["data"] == b""
    assert S.seen_stats(v)["n_rows"] == 0 and sorted(S.seen_add_keys(v, [])) == ["first", "state"] and S.seen_docs(v, [])[0] == []
    assert S.seen_keys(v).dtype == np.uint64 and S.seen_keys(v).size == 0
    S.seen_clear(v)
    S.seen_reserve(v, 0)  # (nothing to make room for beyond what an empty handle has: no table is made)
    assert S.seen_stats(v)["capacity"] == 0 and v.dedup_stats()["n_rows"] == -1


ROW = bytes(range(256)) + bytes(range(255, -1, -1)) + b"tail"


@pytest.mark.parametrize("a,b,same", [
    (ROW, ROW[256:512] + ROW[:256] + ROW[512:], False),  # two chunks swapped: the chunk's index is in its hash
    (b"abc", b"abc\0", False), (b"", b"\0", False), (ROW[:256], ROW[:256] + b"\0", False),  # a trailing zero byte: the length is in it
    (ROW[:255], ROW[:255], True), (b"abcd", b"abdc", False),
], ids=["chunks swapped", "zero byte", "zero byte alone", "zero byte in a new chunk", "equal", "bytes swapped"])
def test_the_key_of_the_model(a, b, same):
    assert (M.key(a) == M.key(b)) == same and 0 < M.key(a) < 2 ** 64
    # the key is a function of the row's bytes alone: the same whatever stands around the row in its batch
    batches = ([a, b], [b"x" * 7, a, b"", b], [b, b"y" * 300, a])
    keys = [dict(zip(rows, M.Seen().add_rows(rows)["keys"])) for rows in batches]
    assert all(k[a] == M.key(a) and k[b] == M.key(b) for k in keys)
    one = M.mix64(M.mix64(((M.S0 ^ 1) + 0x632BE59BD9B4E019) & M.M64) ^ (0x61 | 1 << 32))  # the one chunk of b"a", written out
    assert M.key(b"") == M.mix64(M.S0 ^ 1 << 40) and M.key(b"a") == (M.mix64(M.S0 ^ (1 | 1 << 40)) + one) & M.M64


def test_the_set_of_the_model():
    s = M.Seen()
    assert s.add_keys([5, 0, 5, 1, 7]) == ([0, 0, 1, 1, 0], [0, 1, 0, 1, 4]) and s.export() == [1, 5, 7]
    assert s.add_keys([9, 5, 9], insert=False) == ([0, 2, 1], [0, 1, 0]) and s.export() == [1, 5, 7]
    assert s.stats == dict(n_rows=3, n_new=1, n_repeat_batch=1, n_seen_before=1, n_keys=3)
