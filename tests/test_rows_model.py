"""CPU checks of the documents contract (tests/rows_model.py): one encode of the joined text, cut at the document
starts, gives what one encode per document gives — the claim the library's joined route rests on — and the case where
it does not, which is why the per-document route exists."""
import random

import numpy as np
import pytest

import offsets_model as M
import oracle_lib as O
import rows_model as R
from wordpiece_amd import synth


def test_model_with_tables_built_once_is_the_offsets_model():
    rng = random.Random(21)
    n = 0
    for k in range(400):
        text, vocab = M.random_case(rng)
        if k % 3 == 0:  # duplicate lines: which copy a match names
            vocab = vocab + [vocab[i] for i in range(0, len(vocab), 2)]
            rng.shuffle(vocab)
        try:
            want = M.encode_spans(text, vocab)
        except RuntimeError as e:
            assert "Vocab word is empty" in str(e)
            continue
        assert R.Model(vocab).encode_spans(text) == want, (text, vocab)
        n += 1
    assert n > 350


def random_batch(rng):
    """(documents, vocab): 0..8 documents from random_case (empty ones included), the vocabulary of one more"""
    _, vocab = M.random_case(rng)
    docs = []
    for _ in range(rng.randint(0, 8)):
        docs.append(b"" if rng.random() < 0.15 else M.random_case(rng)[0])
    return docs, vocab


def test_joined_text_cut_at_the_document_starts_equals_per_document():
    rng = random.Random(1234)
    n_docs = n_batches = 0
    for k in range(3000):
        docs, vocab = random_batch(rng)
        try:
            model = R.Model(vocab)
        except RuntimeError as e:  # (the only skip: a vocabulary the model itself rejects)
            assert "Vocab word is empty" in str(e)
            continue
        for unit in ("byte", "char"):
            assert R.encode_rows_joined(model, docs, unit) == R.encode_rows(model, docs, unit), (k, unit, docs, vocab)
        ids, splits, _ = R.encode_rows(model, docs)
        assert ids == model.encode_spans(R.join_docs(docs)[0])[0]  # the rows concatenated: the joined text's ids
        n_docs += len(docs)
        n_batches += 1
    assert n_batches == 3000 and n_docs > 10000


def test_token_with_newline_matches_across_the_separator():
    """fallback 1 on record: with U+000A inside an eligible token the joined text is not the documents"""
    vocab = ["a\nb", "a", "b"]
    model = R.Model(vocab)
    docs = [b"a", b"b"]
    assert R.join_docs(docs) == (b"a\nb\n", [0, 2, 4])
    assert model.encode_spans(b"a\nb\n")[0] == [0]
    assert R.encode_rows(model, docs)[:2] == ([1, 2], [0, 1, 2])
    assert R.encode_rows_joined(model, docs)[0] != R.encode_rows(model, docs)[0]


def test_lines_and_pack_rules():
    assert R.split_lines(b"") == []
    assert R.split_lines(b"\n") == [b""]
    assert R.split_lines(b"a\n\nb") == [b"a", b"", b"b"]
    assert R.split_lines(b"a\n\nb\n") == [b"a", b"", b"b"]
    assert R.join_docs([]) == (b"", [0])
    ids, splits = [5, 6, 7, 8, 9], [0, 3, 3, 5]
    assert R.pack(ids, splits, 4, 101, 102, 0) == ([[101, 5, 6, 102], [101, 102, 0, 0], [101, 8, 9, 102]], [4, 2, 4], 1)
    assert R.pack(ids, splits, 2) == ([[5, 6], [0, 0], [8, 9]], [2, 0, 2], 1)
    assert R.pack(ids, splits, 2, 101, 102, 7) == ([[101, 102]] * 3, [2, 2, 2], 2)
    assert R.pack(ids, splits, 4, None, 102, 7) == ([[5, 6, 7, 102], [102, 7, 7, 7], [8, 9, 102, 7]], [4, 1, 3], 0)
    with pytest.raises(AssertionError):
        R.pack(ids, splits, 1, 101, 102)


def test_oracle_lines_of_an_english_text_concatenate_to_the_whole_text():
    text, vocab = synth.english_corpus(100_000, seed=12, vocab_size=3000)
    ov = O.Vocab(vocab)
    for t in (text.rstrip(b"\n") + b"\n", text.rstrip(b"\n")):
        lines = R.split_lines(t)
        assert len(lines) > 1000
        per_line = [ov.encode(line) if line else np.zeros(0, np.int32) for line in lines]
        assert np.array_equal(np.concatenate(per_line), ov.encode(t))
