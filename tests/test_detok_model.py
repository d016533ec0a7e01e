"""tests/detok_model.py against the tokenizers package (where it is installed), against a recorded fixture of that
package's output (everywhere), and its two forms — plain Python and numpy — against each other.  No GPU."""
import json
import os
import random

import numpy as np
import pytest

import detok_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "detok_tokenizers_cases.json")


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_chain_is_per_token_and_ordered():
    assert M.cleanup(b" do not") == b" don't"
    assert M.cleanup(b" .") == b"." and M.cleanup(b" ' ") == b"'" and M.cleanup(b" n't") == b"n't"
    assert M.piece(b"n't", 1, True) == b"n't" and M.piece(b"n't", 1, False) == b" n't" and M.piece(b"n't", 0, True) == b"n't"
    assert M.piece(b"###", 0, True) == b"###" and M.piece(b"###", 1, True) == b"#"
    assert M.piece(b"##.", 1, True) == b"." and M.piece(b".", 1, True) == b"." and M.piece(b".", 1, False) == b" ."
    # the chain never sees two tokens at once: "do", "not" stay apart, the one token "do not" does not
    m = M.Model(["do", "not", "do not", "x"])
    assert m.strings([3, 0, 1])[0] == b"x do not" and m.strings([3, 2])[0] == b"x don't"


def test_model_equals_recorded_tokenizers_output():
    fx = _fixture()
    m = M.Model(fx["tokens"])
    index = {t: i for i, t in enumerate(fx["tokens"])}
    assert len(fx["cases"]) >= 200
    for case in fx["cases"]:
        ids = [index[t] for t in case["tokens"]]
        assert m.strings(ids, clean=True)[0].decode("utf-8") == case["cleanup"], case
        assert m.strings(ids, clean=False)[0].decode("utf-8") == case["plain"], case


def test_model_equals_tokenizers():
    pytest.importorskip("tokenizers")
    from tokenizers import decoders
    toks = _fixture()["tokens"] + ["##", "## ", " .", " n't", "do  not", "##do", "n'", "t"]
    m = M.Model(toks)
    rng = random.Random(7)
    for clean in (True, False):
        dec = decoders.WordPiece(prefix="##", cleanup=clean)
        for _ in range(4000):
            ids = [rng.randrange(len(toks)) for _ in range(rng.choice([0, 1, 2, 3, 5, 9]))]
            assert m.strings(ids, clean=clean)[0].decode("utf-8") == dec.decode([toks[i] for i in ids]), (clean, ids)


def _random_ragged(rng, V, n_rows, max_row):
    lens = [rng.choice([0, 0, 1, 2, 3, max_row]) if rng.random() < 0.5 else rng.randrange(max_row + 1) for _ in range(n_rows)]
    splits = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.array([rng.choice([-1, V, V + 5, -2 ** 31, 2 ** 31 - 1]) if rng.random() < 0.05 else rng.randrange(V)
                    for _ in range(int(splits[-1]))], dtype=np.int64)
    return ids, splits


def test_plain_and_vectorised_model_agree():
    toks = _fixture()["tokens"]
    m = M.Model(toks, malformed=[toks.index(". ."), toks.index("' '")])
    rng = random.Random(11)
    for trial in range(60):
        ids, splits = _random_ragged(rng, len(toks), rng.choice([1, 2, 7, 40]), rng.choice([1, 3, 9]))
        skip = rng.sample(range(len(toks)), rng.choice([0, 1, 8])) + ([len(toks) + 5] if trial % 3 == 0 else [])
        skip = skip[:8]
        for clean in (True, False):
            for term in (None, "\n", 0):
                text, off, stats = m.detokenize(ids, row_splits=splits, skip_ids=skip, clean=clean, terminator=term)
                t2, o2, s2 = m.detokenize_np(ids, splits, skip_ids=skip, clean=clean, terminator=term)
                assert t2.tobytes() == text and o2.tolist() == off and s2 == stats, (trial, clean, term)


def test_layouts_and_statistics():
    m = M.Model(["[PAD]", "a", "##b", "!!"], malformed=[3])
    # padded: lengths clamp, the cells behind them are no cells
    text, off, st = m.detokenize([[1, 2, 0, 3], [3, 1, 1, 1], [1, 1, 1, 1]], lengths=[9, 2, -4], skip_ids=[0], terminator="\n")
    assert text == b"ab\na\n\n" and off == [0, 3, 5, 6]
    assert st == {"n_rows": 3, "n_cells": 6, "n_kept": 3, "n_skipped": 1, "n_dropped": 2, "n_bytes": 6}
    # ragged, empty rows first, in the middle and last; no terminator
    text, off, st = m.detokenize([2, 1, 1], row_splits=[0, 0, 1, 1, 1, 3, 3])
    assert text == b"##ba a" and off == [0, 0, 3, 3, 3, 6, 6] and st["n_rows"] == 6 and st["n_cells"] == 3
    # a bare 1-d array is one row
    assert m.strings([1, 2, 1]) == [b"ab a"]
