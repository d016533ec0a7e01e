"""CPU checks of the vocabulary learner's entry points (wp_learn_vocab, wp_learn_vocab_device, wp_get_learn_stats):
symbols and structs against the header, what they answer without a device — every argument error with the field it
names, the empty table, the statistics before any call — and that anything else fails loudly without a GPU."""
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
NAMES = ("wp_learn_vocab", "wp_learn_vocab_device", "wp_get_learn_stats")
SPEC_FIELDS = ["reserved_tokens", "reserved_off", "n_reserved", "vocab_size", "lower_thresh", "upper_thresh", "slack", "num_iterations",
               "max_token_chars", "max_unique_chars", "terminator", "hash_bits", "reserved"]
STAT_FIELDS = ["n_words", "n_reserved", "n_long", "n_char_dropped", "n_chars", "n_occurrences", "n_tokens", "n_steps", "thresh", "n_rounds",
               "n_collided"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(W.LIB_PATH):
        from wordpiece_amd import build
        build.build()


def test_symbols_and_structs_match_the_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in W.ABI_SYMBOLS and hasattr(W.lib(), name), name
    assert re.search(r"typedef struct \{ const uint8_t \*reserved_tokens; const int64_t \*reserved_off; int64_t n_reserved, vocab_size, "
                     r"lower_thresh, upper_thresh, slack; int32_t num_iterations, max_token_chars, max_unique_chars, terminator, hash_bits, "
                     r"reserved; \} wp_learn_spec;", hdr)
    assert re.search(r"typedef struct \{ uint8_t \*tokens; int64_t \*token_off, \*scores; int64_t n_tokens, n_bytes, thresh; \} "
                     r"wp_learned_vocab;", hdr)
    assert re.search(r"typedef struct \{ int64_t %s; \} wp_learn_stats;" % ", ".join(STAT_FIELDS), hdr)
    assert [f[0] for f in W.LearnSpec._fields_] == SPEC_FIELDS
    assert [f[0] for f in W.LearnedVocab._fields_] == ["tokens", "token_off", "scores", "n_tokens", "n_bytes", "thresh"]
    assert [(n, C.sizeof(t)) for n, t in W.LearnStats._fields_] == [(n, 8) for n in STAT_FIELDS]
    assert [f[0] for f in W.Stats._fields_][-1] == "rows_route"  # wp_stats keeps its size and its end
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(wp_stats), sizeof(wp_count_stats), sizeof(wp_learn_spec),\n'
                   '         offsetof(wp_learn_spec, n_reserved), offsetof(wp_learn_spec, slack), offsetof(wp_learn_spec, num_iterations),\n'
                   '         offsetof(wp_learn_spec, reserved), sizeof(wp_learned_vocab), offsetof(wp_learned_vocab, n_tokens),\n'
                   '         offsetof(wp_learned_vocab, thresh), sizeof(wp_learn_stats), offsetof(wp_learn_stats, n_collided));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(W.Stats), C.sizeof(W.CountStats), C.sizeof(W.LearnSpec), W.LearnSpec.n_reserved.offset, W.LearnSpec.slack.offset,
                   W.LearnSpec.num_iterations.offset, W.LearnSpec.reserved.offset, C.sizeof(W.LearnedVocab), W.LearnedVocab.n_tokens.offset,
                   W.LearnedVocab.thresh.offset, C.sizeof(W.LearnStats), W.LearnStats.n_collided.offset]
    assert C.sizeof(W.LearnSpec) == 80 and C.sizeof(W.LearnedVocab) == 48 and C.sizeof(W.LearnStats) == 88 and C.sizeof(W.CountStats) == 56


RES = b"[PAD][UNK]"
RES_OFF = (C.c_int64 * 3)(0, 5, 10)


def _spec(res=RES, res_off=RES_OFF, n_reserved=2, vocab_size=100, lower_thresh=1, upper_thresh=100, slack=5, num_iterations=4,
          max_token_chars=50, max_unique_chars=1000, terminator=-1, hash_bits=0, reserved=0):
    return W.LearnSpec(res, res_off, n_reserved, vocab_size, lower_thresh, upper_thresh, slack, num_iterations, max_token_chars,
                       max_unique_chars, terminator, hash_bits, reserved)


WORDS = np.frombuffer(b"abba", dtype=np.uint8)
OFF = np.array([0, 2, 4], dtype=np.int64)
CNT = np.array([3, 1], dtype=np.int64)


def _host(v, spec, n=2, out=True, words=WORDS, off=OFF, cnt=CNT):
    o = W.LearnedVocab(1, 2, 3, 4, 5, 6)  # (garbage in: the call clears it)
    rc = W.lib().wp_learn_vocab(v._h, words.ctypes.data if words is not None else None, off.ctypes.data if off is not None else None,
                                cnt.ctypes.data if cnt is not None else None, n, None if spec is None else C.byref(spec),
                                C.byref(o) if out else None)
    return rc, o


def _device(v, spec, n=2, out=True, nbytes=4, off=512, cnt=1024):
    """the device form with pointers that are never dereferenced: the argument rules come first"""
    o = W.LearnedVocab(1, 2, 3, 4, 5, 6)
    rc = W.lib().wp_learn_vocab_device(v._h, C.c_void_p(256), nbytes, C.c_void_p(off), C.c_void_p(cnt), n,
                                       None if spec is None else C.byref(spec), C.byref(o) if out else None)
    return rc, o


def _cleared(o):
    return not (o.tokens or o.token_off or o.scores) and (o.n_tokens, o.n_bytes, o.thresh) == (0, 0, 0)


def test_argument_errors_come_before_the_device_and_name_the_field():
    L = W.lib()
    v = W.Vocab(VOCAB)
    assert v.learn_stats()["n_words"] == -1  # a fresh handle: no such call yet
    empty_off, nl_off = (C.c_int64 * 3)(0, 5, 5), (C.c_int64 * 2)(0, 3)
    cases = [(None, b"spec is NULL"), (_spec(vocab_size=0), b"vocab_size"), (_spec(max_token_chars=0), b"max_token_chars"),
             (_spec(max_token_chars=65), b"max_token_chars"), (_spec(num_iterations=0), b"num_iterations"),
             (_spec(lower_thresh=0), b"lower_thresh"), (_spec(upper_thresh=0), b"upper_thresh"),
             (_spec(lower_thresh=9, upper_thresh=8), b"lower_thresh"), (_spec(slack=-1), b"slack"),
             (_spec(max_unique_chars=-1), b"max_unique_chars"), (_spec(terminator=256), b"terminator"), (_spec(terminator=-2), b"terminator"),
             (_spec(hash_bits=7), b"hash_bits"), (_spec(hash_bits=65), b"hash_bits"), (_spec(reserved=1), b"reserved must be 0"),
             (_spec(n_reserved=-1), b"n_reserved"), (_spec(res=None), b"reserved_tokens"), (_spec(res_off=None), b"reserved_off"),
             (_spec(res_off=empty_off), b"reserved_tokens: token 1 is empty"), (_spec(res=b"a\nb", res_off=nl_off, n_reserved=1), b"line feed")]
    for spec, msg in cases:
        for n in (2, 0):
            rc, o = _host(v, spec, n=n)
            assert rc == ARG and msg in L.wp_last_error() and _cleared(o), (msg, L.wp_last_error())
        rc, o = _device(v, spec)
        assert rc == ARG and msg in L.wp_last_error() and _cleared(o), (msg, L.wp_last_error())
    for call in (lambda: _host(v, _spec(), out=False), lambda: _device(v, _spec(), out=False)):
        assert call()[0] == ARG and b"out is NULL" in L.wp_last_error()
    # the table's pointers, sizes and alignment
    assert _host(v, _spec(), off=None)[0] == ARG and b"word_off is NULL" in L.wp_last_error()
    assert _host(v, _spec(), cnt=None)[0] == ARG and b"counts is NULL" in L.wp_last_error()
    assert _host(v, _spec(), words=None)[0] == ARG and b"words is NULL" in L.wp_last_error()
    assert _host(v, _spec(), off=np.array([0, 2, -4], dtype=np.int64))[0] == ARG and b"word_off" in L.wp_last_error()
    assert _host(v, _spec(), off=np.array([0, 2, 2 ** 32], dtype=np.int64))[0] == TOO_LARGE and b"UINT32_MAX" in L.wp_last_error()
    assert _device(v, _spec(), nbytes=2 ** 32)[0] == TOO_LARGE and b"UINT32_MAX" in L.wp_last_error()
    assert _device(v, _spec(), n=2 ** 31)[0] == TOO_LARGE and b"2^31 words" in L.wp_last_error()
    assert _device(v, _spec(), off=516)[0] == ARG and b"word_off must be 8-byte aligned" in L.wp_last_error()
    assert _device(v, _spec(), cnt=1028)[0] == ARG and b"counts must be 8-byte aligned" in L.wp_last_error()
    assert v.learn_stats()["n_words"] == -1  # none of these was a call
    # the Python mirror's own rules
    with pytest.raises(W.WordPieceError, match="one entry more"):
        v.learn_vocab({"words": ["a", "b"], "counts": [1]}, 10)
    with pytest.raises(W.WordPieceError, match="max_token_chars"):
        v.learn_vocab({"words": [], "counts": []}, 10, max_token_chars=100)


def test_empty_table_needs_no_device():
    v = W.Vocab(VOCAB)
    for spec in (_spec(), _spec(terminator=10, hash_bits=8, slack=0, max_unique_chars=0)):
        rc, o = _host(v, spec, n=0, words=None, off=None, cnt=None)
        assert rc == 0 and (o.n_tokens, o.n_bytes, o.thresh) == (2, 12, 0)
        assert C.string_at(o.tokens, 12) == b"[PAD]\n[UNK]\n"
        assert C.cast(o.token_off, C.POINTER(C.c_int64))[0:3] == [0, 6, 12] and C.cast(o.scores, C.POINTER(C.c_int64))[0:2] == [0, 0]
        for blk in (o.tokens, o.token_off, o.scores):
            W.lib().wp_free(blk)
        assert v.learn_stats() == dict.fromkeys(STAT_FIELDS, 0)
    rc, o = _host(v, _spec(n_reserved=0), n=0, words=None, off=None, cnt=None)
    assert rc == 0 and o.token_off and not (o.tokens or o.scores) and (o.n_tokens, o.n_bytes) == (0, 0)
    W.lib().wp_free(o.token_off)
    r = v.learn_vocab({"words": [], "counts": []}, 10)
    assert r["tokens"] == list(W.DEFAULT_RESERVED) and r["scores"].tolist() == [0] * 5 and r["thresh"] == 0
    assert v.learn_vocab({"words": np.zeros(0, np.uint8), "word_off": [0], "counts": [], "terminator": "\n"}, 10, reserved=())["tokens"] == []


def test_no_cpu_fallback():
    if W.lib().wp_device_count() > 0:
        pytest.skip("GPU present")
    v = W.Vocab(VOCAB)
    L = W.lib()
    rc, o = _host(v, _spec())
    assert rc == NO_DEVICE and b"no HIP device" in L.wp_last_error() and _cleared(o)
    assert _device(v, _spec())[0] == NO_DEVICE and b"no HIP device" in L.wp_last_error()
    assert _device(v, _spec(), n=0, nbytes=0)[0] == NO_DEVICE  # (the device form keeps even the empty list in device memory)
    with pytest.raises(W.WordPieceError, match="no HIP device"):
        v.learn_vocab({"words": ["ab", "ba"], "counts": [3, 1]}, 10)
