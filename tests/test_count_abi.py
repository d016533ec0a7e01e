"""CPU checks of the word-count entry points (wp_count_words, wp_count_words_device, wp_get_count_stats): symbols and
structs against the header, what they answer without a device — every argument error with the field it names, the empty
text, the statistics before any call — and that anything else fails loudly without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import wordpiece_amd as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = ["[UNK]", "a", "b"]
ARG, TOO_LARGE, NO_DEVICE = 6, 2, 4
NAMES = ("wp_count_words", "wp_count_words_device", "wp_get_count_stats")
STAT_FIELDS = ["n_words", "n_distinct", "n_long", "n_below_min", "n_text_bytes", "n_rounds", "n_collided"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(W.LIB_PATH):
        from wordpiece_amd import build
        build.build()


def test_symbols_and_structs_match_the_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in W.ABI_SYMBOLS and hasattr(W.lib(), name), name
    assert re.search(r"typedef struct \{ int32_t order, max_word_bytes, terminator, want, hash_bits, reserved; int64_t min_count; \} "
                     r"wp_count_spec;", hdr)
    assert re.search(r"typedef struct \{ uint8_t \*words; int64_t \*word_off, \*counts; int32_t \*word_index; int64_t n_distinct, n_words, "
                     r"n_bytes; \} wp_word_counts;", hdr)
    assert re.search(r"typedef struct \{ int64_t %s; \} wp_count_stats;" % ", ".join(STAT_FIELDS), hdr)
    for macro, value in (("WP_COUNT_ORDER_FIRST", 0), ("WP_COUNT_ORDER_COUNT", 1), ("WP_COUNT_WANT_INDEX", 1)):
        assert re.search(r"#define %s\s+%d\b" % (macro, value), hdr) and getattr(W, macro) == value
    assert [f[0] for f in W.CountSpec._fields_] == ["order", "max_word_bytes", "terminator", "want", "hash_bits", "reserved", "min_count"]
    assert [f[0] for f in W.WordCounts._fields_] == ["words", "word_off", "counts", "word_index", "n_distinct", "n_words", "n_bytes"]
    assert [(n, C.sizeof(t)) for n, t in W.CountStats._fields_] == [(n, 8) for n in STAT_FIELDS]
    assert [f[0] for f in W.Stats._fields_][-1] == "rows_route"  # wp_stats keeps its size and its end
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(wp_stats), sizeof(wp_count_spec),\n'
                   '         offsetof(wp_count_spec, hash_bits), offsetof(wp_count_spec, min_count), sizeof(wp_word_counts),\n'
                   '         offsetof(wp_word_counts, word_index), offsetof(wp_word_counts, n_distinct), offsetof(wp_word_counts, n_bytes),\n'
                   '         sizeof(wp_count_stats), offsetof(wp_count_stats, n_collided));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(W.Stats), C.sizeof(W.CountSpec), W.CountSpec.hash_bits.offset, W.CountSpec.min_count.offset,
                   C.sizeof(W.WordCounts), W.WordCounts.word_index.offset, W.WordCounts.n_distinct.offset, W.WordCounts.n_bytes.offset,
                   C.sizeof(W.CountStats), W.CountStats.n_collided.offset]
    assert C.sizeof(W.CountSpec) == 32 and C.sizeof(W.WordCounts) == 56 and C.sizeof(W.CountStats) == 56


def _spec(order=0, max_word_bytes=0, terminator=-1, want=0, hash_bits=0, reserved=0, min_count=0):
    return W.CountSpec(order, max_word_bytes, terminator, want, hash_bits, reserved, min_count)


def _host(v, text, spec, out=True):
    o = W.WordCounts(1, 2, 3, 4, 5, 6, 7)  # (garbage in: the call clears it)
    rc = W.lib().wp_count_words(v._h, text, len(text), None if spec is None else C.byref(spec), C.byref(o) if out else None)
    return rc, o


def _device(v, spec, nbytes=8, out=True):
    """the device form with a pointer that is never dereferenced: the argument rules come first"""
    o = W.WordCounts(1, 2, 3, 4, 5, 6, 7)
    rc = W.lib().wp_count_words_device(v._h, C.c_void_p(256), nbytes, None if spec is None else C.byref(spec), C.byref(o) if out else None)
    return rc, o


def _cleared(o):
    return not (o.words or o.word_off or o.counts or o.word_index) and (o.n_distinct, o.n_words, o.n_bytes) == (0, 0, 0)


def test_argument_errors_come_before_the_device_and_name_the_field():
    L = W.lib()
    v = W.Vocab(VOCAB)
    assert v.count_stats()["n_words"] == -1  # a fresh handle: no such call yet
    cases = [(None, b"spec is NULL"), (_spec(order=2), b"order"), (_spec(order=-1), b"order"), (_spec(want=2), b"want"),
             (_spec(want=-1), b"want"), (_spec(terminator=256), b"terminator"), (_spec(terminator=-2), b"terminator"),
             (_spec(hash_bits=7), b"hash_bits"), (_spec(hash_bits=65), b"hash_bits"), (_spec(hash_bits=-1), b"hash_bits"),
             (_spec(max_word_bytes=1025), b"max_word_bytes"), (_spec(max_word_bytes=-1), b"max_word_bytes"),
             (_spec(min_count=-1), b"min_count"), (_spec(reserved=1), b"reserved")]
    for spec, msg in cases:
        for text in (b"a b a", b""):
            rc, o = _host(v, text, spec)
            assert rc == ARG and msg in L.wp_last_error() and _cleared(o), (msg, L.wp_last_error())
        rc, o = _device(v, spec)
        assert rc == ARG and msg in L.wp_last_error() and _cleared(o), (msg, L.wp_last_error())
    for call in (lambda: _host(v, b"a", _spec(), out=False), lambda: _device(v, _spec(), out=False)):
        assert call()[0] == ARG and b"out is NULL" in L.wp_last_error()
    # the size, the text pointer and its alignment
    o = W.WordCounts()
    assert L.wp_count_words(v._h, b"a", 2 ** 32, C.byref(_spec()), C.byref(o)) == TOO_LARGE and b"UINT32_MAX" in L.wp_last_error()
    assert _device(v, _spec(), nbytes=2 ** 32)[0] == TOO_LARGE and b"UINT32_MAX" in L.wp_last_error()
    assert L.wp_count_words(v._h, None, 3, C.byref(_spec()), C.byref(o)) == ARG and b"utf8 is NULL" in L.wp_last_error()
    assert L.wp_count_words_device(v._h, C.c_void_p(257), 8, C.byref(_spec()), C.byref(o)) == ARG and b"aligned" in L.wp_last_error()
    assert v.count_stats()["n_words"] == -1  # none of these was a call
    # the Python mirror's own rules
    for kw in (dict(order="alpha"), dict(terminator="ab")):
        with pytest.raises(W.WordPieceError):
            v.count_words("a", **kw)
    with pytest.raises(W.WordPieceError, match="max_word_bytes"):
        v.count_words("", max_word_bytes=2000)


def test_empty_text_needs_no_device():
    v = W.Vocab(VOCAB)
    for spec in (_spec(), _spec(order=1, want=1, terminator=10, min_count=3, hash_bits=8, max_word_bytes=1)):
        rc, o = _host(v, b"", spec)
        assert rc == 0 and o.word_off and not (o.words or o.counts or o.word_index) and (o.n_distinct, o.n_words, o.n_bytes) == (0, 0, 0)
        assert C.cast(o.word_off, C.POINTER(C.c_int64))[0] == 0
        W.lib().wp_free(o.word_off)
        assert v.count_stats() == dict.fromkeys(STAT_FIELDS, 0)
    r = v.count_words("", index=True)
    assert r["words"] == [] and r["counts"].dtype == np.int64 and r["counts"].shape == (0,) and r["word_index"].shape == (0,)
    r = v.count_words(b"", raw=True, terminator="\n", order="count")
    assert r["words"].shape == (0,) and r["word_off"].tolist() == [0] and "word_index" not in r


def test_no_cpu_fallback():
    if W.lib().wp_device_count() > 0:
        pytest.skip("GPU present")
    v = W.Vocab(VOCAB)
    L = W.lib()
    for text in (b"a b a", b" ", b"\xff"):
        rc, o = _host(v, text, _spec())
        assert rc == NO_DEVICE and b"no HIP device" in L.wp_last_error() and _cleared(o)
    assert _device(v, _spec())[0] == NO_DEVICE and b"no HIP device" in L.wp_last_error()
    assert _device(v, _spec(), nbytes=0)[0] == NO_DEVICE  # (the device form keeps even the empty table in device memory)
    with pytest.raises(W.WordPieceError, match="no HIP device"):
        v.count_words("a b a")
