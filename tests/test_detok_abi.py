"""The detokenize entry points through the C ABI, without a GPU: wp_detok_piece against the model for every id, form
and cleanup value, against the recorded tokenizers fixture, and every argument rule the host entry point checks before
it touches a device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import detok_model as M
import wordpiece_amd as W

HERE = os.path.dirname(os.path.abspath(__file__))
LONG = "q" * 1500
# 1-, 2-, 3- and 4-byte tokens and their continuations, the clean-up tokens, an inner space, "###", specials, a
# malformed line ("!!": punctuation only, longer than one)
VOCAB = ["[UNK]", "[CLS]", "[SEP]", "[PAD]", "[MASK]", "a", "##a", "é", "##é", "中", "##中", "\U0001f600",
         "##\U0001f600", ".", "##.", ",", "?", "!", "'", "n't", "##n't", "'m", "'s", "'ve", "'re", "do not", "##do not",
         "do", "not", "x y", "###", "#", "!!", "café", "is n't", LONG, "##" + LONG]
MALFORMED = VOCAB.index("!!")
WP_ERR_TOO_LARGE, WP_ERR_ARG = 2, 6


@pytest.fixture(scope="module")
def vocab():
    return W.Vocab(VOCAB)


@pytest.fixture(scope="module")
def model(vocab):
    return M.Model.from_vocab(vocab)


def test_model_sees_the_vocabulary_as_given(vocab, model):
    assert model.lines == [t.encode("utf-8") for t in VOCAB] and model.malformed == {MALFORMED}


def test_piece_equals_model_for_every_id(vocab, model):
    n = 0
    for i in range(len(VOCAB)):
        for form in (0, 1):
            for clean in (False, True):
                assert vocab.detok_piece(i, form, clean) == model.piece(i, form, clean), (i, form, clean)
                n += 1
    assert n == 4 * len(VOCAB) and vocab.detok_piece(MALFORMED, 0) is None
    assert vocab.detok_piece(VOCAB.index("do not"), 1, True) == b" don't"
    assert vocab.detok_piece(VOCAB.index("###"), 1, True) == b"#"


def test_piece_rejects_and_truncates(vocab):
    L = W.lib()
    for i, form, clean in ((-1, 0, 1), (len(VOCAB), 0, 1), (5, 2, 1), (5, -1, 1), (5, 0, 2), (5, 0, -1), (MALFORMED, 1, 0)):
        assert L.wp_detok_piece(vocab._h, i, form, clean, None, 0) == -1
    buf = C.create_string_buffer(b"zzzzzzzz")
    assert L.wp_detok_piece(vocab._h, VOCAB.index("do not"), 1, 0, buf, 3) == 7 and buf.raw == b" dozzzzz\0"


def test_piece_equals_recorded_tokenizers_output():
    with open(os.path.join(HERE, "golden", "detok_tokenizers_cases.json")) as f:
        fx = json.load(f)
    v = W.Vocab(fx["tokens"])
    bad = {i for i in range(len(v)) if v.token_flags(i) & 4}
    index = {t: i for i, t in enumerate(fx["tokens"])}
    used = 0
    for case in fx["cases"]:
        ids = [index[t] for t in case["tokens"]]
        if bad & set(ids):
            continue
        for clean, key in ((True, "cleanup"), (False, "plain")):
            got = b"".join(v.detok_piece(i, 0 if k == 0 else 1, clean) for k, i in enumerate(ids))
            assert got.decode("utf-8") == case[key], case
        used += 1
    assert used >= 150


def _call(vocab, ids, splits, lengths, n_rows, spec, outs=(True, True, True)):
    text, off, nb = C.c_void_p(), C.POINTER(C.c_int64)(), C.c_size_t(77)
    rc = W.lib().wp_detokenize(vocab._h, ids, splits, lengths, n_rows, None if spec is None else C.byref(spec),
                               C.byref(text) if outs[0] else None, C.byref(off) if outs[1] else None,
                               C.byref(nb) if outs[2] else None)
    return rc, text, off, nb


def _spec(max_len=0, cleanup=1, terminator=-1, n_skip=0):
    return W.DetokSpec(max_len, cleanup, terminator, n_skip, (C.c_int32 * 8)())


def test_argument_errors_need_no_device(vocab):
    ids = (C.c_int32 * 4)(5, 6, 5, 6)
    ok_splits = (C.c_int64 * 3)(0, 2, 4)
    assert W.lib().wp_get_detok_stats  # (the symbol exists)
    bad = [
        (ids, ok_splits, None, 2, None),
        (ids, ok_splits, None, 2, _spec(cleanup=2)),
        (ids, ok_splits, None, 2, _spec(cleanup=-1)),
        (ids, ok_splits, None, 2, _spec(terminator=-2)),
        (ids, ok_splits, None, 2, _spec(terminator=256)),
        (ids, ok_splits, None, 2, _spec(n_skip=-1)),
        (ids, ok_splits, None, 2, _spec(n_skip=9)),
        (ids, ok_splits, None, 2, _spec(max_len=-1)),
        (ids, None, None, 2, _spec()),                                  # ragged without row_splits
        (None, ok_splits, None, 2, _spec()),                            # cells without ids
        (None, None, None, 2, _spec(max_len=2)),
        (ids, (C.c_int64 * 3)(1, 2, 4), None, 2, _spec()),              # does not start at 0
        (ids, (C.c_int64 * 3)(0, 3, 2), None, 2, _spec()),              # descends
        (ids, (C.c_int64 * 3)(0, -1, 2), None, 2, _spec()),
    ]
    for k, (a, s, l, n, sp) in enumerate(bad):
        rc, text, off, nb = _call(vocab, a, s, l, n, sp)
        assert rc == WP_ERR_ARG, (k, rc)
        assert not text.value and not off and nb.value == 0 and W.lib().wp_last_error()
    for outs in ((False, True, True), (True, False, True), (True, True, False)):
        assert _call(vocab, ids, ok_splits, None, 2, _spec(), outs)[0] == WP_ERR_ARG


def test_size_errors_need_no_device(vocab):
    ids = (C.c_int32 * 4)(5, 6, 5, 6)
    # the size rules come before any pointer is read: the arrays are far shorter than the counts say
    assert _call(vocab, ids, (C.c_int64 * 3)(0, 2, 4), None, 2 ** 31, _spec())[0] == WP_ERR_TOO_LARGE
    assert _call(vocab, ids, None, None, 2 ** 31, _spec(max_len=1))[0] == WP_ERR_TOO_LARGE
    assert _call(vocab, ids, None, None, 2 ** 16, _spec(max_len=2 ** 15))[0] == WP_ERR_TOO_LARGE      # 2^31 cells
    assert _call(vocab, ids, None, None, 2 ** 31 - 1, _spec(max_len=2 ** 31 - 1))[0] == WP_ERR_TOO_LARGE
    assert _call(vocab, ids, (C.c_int64 * 2)(0, 2 ** 31), None, 1, _spec())[0] == WP_ERR_TOO_LARGE   # 2^31 cells, ragged
    assert _call(vocab, ids, (C.c_int64 * 2)(0, 2 ** 40), None, 1, _spec())[0] == WP_ERR_TOO_LARGE


def test_no_rows_needs_no_device():
    v = W.Vocab(VOCAB)
    assert v.detok_stats()["n_rows"] == -1                     # no such call yet
    for spec, splits in ((_spec(), (C.c_int64 * 1)(0)), (_spec(max_len=3, terminator=10), None)):
        rc, text, off, nb = _call(v, None, splits, None, 0, spec)
        assert rc == 0 and not text.value and nb.value == 0 and off[0] == 0
        W.lib().wp_free(off)
        assert v.detok_stats() == {"n_rows": 0, "n_cells": 0, "n_kept": 0, "n_skipped": 0, "n_dropped": 0, "n_bytes": 0}
    assert v.detokenize(np.zeros(0, np.int32), row_splits=[0]) == []
    assert v.detokenize(np.zeros((0, 5), np.int32)) == []
    assert v.stats()["n_ids"] == 0                             # the encode statistics are not this call's


def test_python_mirror_rejects_before_the_library(vocab):
    with pytest.raises(W.WordPieceError):
        vocab.detokenize([1, 2], row_splits=[0, 3])
    with pytest.raises(W.WordPieceError):
        vocab.detokenize([[1, 2]], row_splits=[0, 2])
    with pytest.raises(W.WordPieceError):
        vocab.detokenize([1, 2], lengths=[2])
    with pytest.raises(W.WordPieceError):
        vocab.detokenize([1, 2], skip_ids=range(9))
    with pytest.raises(W.WordPieceError):
        vocab.detokenize([1, 2], terminator="ab")
    assert C.sizeof(W.DetokSpec) == 48 and C.sizeof(W.DetokStats) == 48
