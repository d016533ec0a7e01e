"""CPU tests of the offsets model (tests/offsets_model.py) and of the offsets entry points without a device: the
model's ids are the C oracle's, its spans satisfy what include/wordpiece_amd.h promises."""
import json
import os
import random

import numpy as np
import pytest

import offsets_model as M
import oracle_lib as O
import wordpiece_amd as W

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)["cases"]


def _golden():
    for name in ("reference_tests_cpp.json", "survey_probed_cases.json"):
        for case in _load(name):
            yield bytes.fromhex(case["text_hex"]), [bytes.fromhex(w) for w in case["vocab_hex"]]


def _check(text, vocab):
    ids, spans, t, starts = M.encode_spans(text, vocab)
    assert ids == O.encode(text, vocab).tolist(), (text, vocab)
    M.check_coverage(text, ids, spans, t, starts)
    return ids, spans


def test_model_matches_oracle_on_golden_vectors():
    n = 0
    for text, vocab in _golden():
        try:
            O.Vocab(vocab)
        except O.OracleError:
            continue
        _check(text, vocab)
        n += 1
    assert n > 10


def test_model_matches_oracle_random():
    rng = random.Random(2024)
    unk_spans = 0
    for _ in range(1500):
        text, vocab = M.random_case(rng)
        ids, spans = _check(text, vocab)
        unk = vocab.index(b"[UNK]") if b"[UNK]" in vocab else -1
        unk_spans += sum(1 for i, (b, e) in zip(ids, spans) if i == unk and e - b > 1)
    assert unk_spans > 50  # the cases reach [UNK]s that replace words of several characters


def test_model_spans_by_hand():
    vocab = ["[UNK]", "un", "##aff", "##able", "a", "-", "中"]
    text = "  unaffable xyz a-中 unaffx"
    ids, offs = M.encode_with_offsets(text, vocab, unit="char")
    assert ids == [1, 2, 3, 0, 4, 5, 6, 0]
    assert offs == [(2, 4), (4, 7), (7, 11), (12, 15), (16, 17), (17, 18), (18, 19), (20, 26)]
    ids_b, offs_b = M.encode_with_offsets(text, vocab, unit="byte")
    assert ids_b == ids
    assert offs_b[6] == (18, 21) and offs_b[7] == (22, 28)
    # an invalid byte inside a word belongs to its span, one between words to none
    ids, offs = M.encode_with_offsets(b"a\xffa \xff a", ["a", "##a"], unit="byte")
    assert ids == [0, 1, 0] and offs == [(0, 1), (2, 3), (6, 7)]


def test_empty_text_needs_no_device():
    v = W.Vocab(["a", "##b"])
    for unit in ("byte", "char"):
        ids, offs = v.encode_with_offsets(b"", unit=unit)
        assert ids.dtype == np.int32 and ids.shape == (0,)
        assert offs.dtype == np.uint32 and offs.shape == (0, 2)


def test_bad_unit_is_an_argument_error():
    v = W.Vocab(["a"])
    import ctypes as C
    ids, offs, n = C.POINTER(C.c_int32)(), C.POINTER(C.c_uint32)(), C.c_size_t()
    assert W.lib().wp_linear_encode_offsets(v._h, b"a", 1, 2, C.byref(ids), C.byref(offs), C.byref(n)) == 6  # WP_ERR_ARG
    with pytest.raises(W.WordPieceError):
        v.encode_with_offsets(b"a", unit="word")


def test_no_cpu_fallback():
    if W.lib().wp_device_count() > 0:
        pytest.skip("GPU present")
    import ctypes as C
    v = W.Vocab(["a", "##b"])
    ids, offs, n = C.POINTER(C.c_int32)(), C.POINTER(C.c_uint32)(), C.c_size_t()
    for unit in (0, 1):
        assert W.lib().wp_linear_encode_offsets(v._h, b"ab", 2, unit, C.byref(ids), C.byref(offs), C.byref(n)) == 4
    d_ids, d_offs = C.c_void_p(), C.c_void_p()
    buf = (C.c_uint32 * 4)()
    assert W.lib().wp_linear_encode_offsets_device(v._h, C.cast(buf, C.c_void_p), 2, 0, C.byref(d_ids), C.byref(d_offs),
                                                   C.byref(n)) == 4
    with pytest.raises(W.WordPieceError, match="no HIP device"):
        v.encode_with_offsets("ab")


def test_model_duplicate_lines_match_oracle():
    """Duplicate vocab lines: the reference takes the copy its suffix order puts next to the text position (the model
    states the rule); a text that ends in a duplicated token is the case where the order is not the plain one."""
    rng = random.Random(99)
    n = 0
    for _ in range(1500):
        alpha = "ab -"
        v = ["".join(rng.choice(alpha) for _ in range(rng.randint(1, 3))) for _ in range(rng.randint(1, 8))]
        v = [w if rng.random() < 0.6 else "##" + w for w in v]
        v = [w for w in v if w.strip() and w != "##"] or ["a"]
        v += [rng.choice(v) for _ in range(rng.randint(1, 3))]
        t = "".join(rng.choice(alpha) for _ in range(rng.randint(1, 14)))
        try:
            exp = O.encode(t, v).tolist()
        except O.OracleError:
            continue
        assert M.encode_spans(t, v)[0] == exp, (t, v)
        n += 1
    assert n > 1000
    assert M.encode_spans("ab ab", ["ab", "x", "ab"])[0] == O.encode("ab ab", ["ab", "x", "ab"]).tolist() == [0, 0]
