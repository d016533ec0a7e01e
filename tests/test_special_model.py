"""tests/special_model.py against a recorded fixture of the `tokenizers` package's output (everywhere), against the
package itself (where it is installed), and its two statements — blank-and-merge and segment by segment — against each
other.  No GPU."""
import json
import os
import random

import pytest

import offsets_model as OM
import rows_model as R
import special_model as S
from bruteforce import is_space

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "special_tokenizers_cases.json")


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_eligible_lines():
    yes = ["[MASK]", "[a]", "[UNK]", "[MASK2]", "[a.b]", "[" + "x" * 62 + "]", "[#a]"]
    no = ["[]", "[.]", "[..]", "MASK", "[MASK", "MASK]", "##[a]", "[a b]", "[a[b]", "[a]b]", "[é]", "[a\x7f]", "[a\x01]",
          "[" + "x" * 63 + "]", "[[a]", "[a]]", " [a]"]
    for w in yes:
        assert S.eligible_line(w), w
    for w in no:
        assert not S.eligible_line(w), w
    vocab = ["[UNK]", "a", "[MASK]", "[.]", "[MASK]", "[a b]", "[SEP]"]
    assert S.special_ids(vocab) == [0, 2, 6]
    assert S.special_ids(vocab, ["[SEP]", "[MASK]"]) == [6, 2]


def test_table_errors_name_the_id():
    vocab = ["[UNK]", "a", "[MASK]", "[.]", "[MASK]", "[a b]"]
    assert S.table(vocab, [2, 0, 2]) == {b"[MASK]": 2, b"[UNK]": 0}
    for ids, word in (([6], "6"), ([-1], "-1"), ([1], "1"), ([3], "3"), ([5], "5"), ([2, 4], "4"), ([4, 0, 2], "2")):
        with pytest.raises(ValueError, match=r"id %s\b" % word):
            S.table(vocab, ids)
    with pytest.raises(ValueError):
        S.table(vocab, [0] * 4097)
    assert len(S.table(vocab, [0] * 4096)) == 1


def test_find_is_maximal_and_decided_by_the_text():
    tab = S.table(["[MASK]", "[a]", "[" + "x" * 62 + "]"], [0, 1, 2])
    f = lambda t: [(p, l) for p, l, _ in S.find(t, tab)]
    assert f("[MASK]") == [(0, 6)] and f("x[MASK]") == [(1, 6)] and f("[MASK][a]") == [(0, 6), (6, 3)]
    assert f("[[MASK]]") == [(1, 6)] and f("[mask]") == [] and f("[MASK") == [] and f("[MA SK]") == [] and f("[MASK2]") == []
    assert f("[a[a]") == [(2, 3)] and f("[" * 9) == [] and f("[MAS\xc3\xa9K]") == []
    assert f("[" + "x" * 62 + "]") == [(0, 64)] and f("[" + "x" * 63 + "]") == []
    assert S.blank(b"a[a]b", S.find(b"a[a]b", tab)) == b"a   b"


def test_model_equals_recorded_tokenizers_output():
    fx = _fixture()
    model = R.Model(fx["vocab"])
    tab = S.table(fx["vocab"], S.special_ids(fx["vocab"], fx["specials"]))
    assert sorted(tab.values()) == S.special_ids(fx["vocab"])
    assert len(fx["cases"]) >= 400
    n_literals = 0
    for case in fx["cases"]:
        ids, offs = S.encode_special(model, case["text"], tab, "char")
        assert ids == case["ids"], case
        assert [list(o) for o in offs] == case["offsets"], case
        n_literals += len(S.find(case["text"], tab))
    assert n_literals >= 400
    # the case the issue starts from: without the list "[CLS] a" falls apart, with it the id stands
    assert S.encode_special(model, "[CLS] a", {}, None)[0] == [10, 0, 11, 17]
    assert S.encode_special(model, "[CLS] a", tab, None)[0] == [1, 17]


def test_model_equals_tokenizers():
    pytest.importorskip("tokenizers")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_special", os.path.join(HERE, "golden", "make_special_tokenizers_cases.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    tok = gen.make_tokenizer()
    model = R.Model(gen.VOCAB)
    tab = S.table(gen.VOCAB, S.special_ids(gen.VOCAB, gen.SPECIALS))
    rng = random.Random(11)
    n_literals = 0
    for _ in range(3000):
        text = gen.random_text(rng)
        e = tok.encode(text, add_special_tokens=False)
        ids, offs = S.encode_special(model, text, tab, "char")
        assert ids == e.ids and offs == [tuple(o) for o in e.offsets], text
        n_literals += len(S.find(text, tab))
    assert n_literals >= 3000


def _random_case(rng):
    """(text, vocab, listed ids): a vocabulary without blanks, U+0000 or U+0001 in its tokens and without duplicate
    lines, with special lines some of which are listed; a text that mixes its words with literals and near-literals"""
    text, vocab = OM.random_case(rng)
    vocab = [w for w in dict.fromkeys(vocab) if not any(is_space(c) or c < 2 for c in OM.decode_with_starts(w)[0])]
    specials = [b"[MASK]", b"[SEP]", b"[a]", b"[ab-c]", b"[" + b"q" * 62 + b"]"]
    rng.shuffle(specials)
    specials = specials[:rng.randint(1, 5)]
    vocab += specials + [b"[", b"]"][:rng.randint(0, 2)]
    if not any(w for w in vocab if not w.startswith(b"[")):
        vocab.append(b"a")
    rng.shuffle(vocab)
    listed = [vocab.index(w) for w in specials if rng.random() < 0.8]
    near = [b"[", b"]", b"[MASK", b"MASK]", b"[mask]", b"[MA SK]", b"[[", b"]]", b"[" + b"q" * 63 + b"]", b"\n", b" "]
    words = [text[i:i + rng.randint(1, 6)] for i in range(0, len(text), 6)] or [b"a"]
    parts = []
    for _ in range(rng.randint(1, 14)):
        r = rng.random()
        parts.append(rng.choice(specials) if r < 0.4 else rng.choice(near) if r < 0.6 else rng.choice(words))
    return b"".join(parts), vocab, listed


def test_blank_and_merge_equals_segment_by_segment():
    rng = random.Random(20261019)
    n_literals = 0
    for k in range(3000):
        text, vocab, listed = _random_case(rng)
        model = R.Model(vocab)
        tab = S.table(vocab, listed)
        ids, offs = S.encode_special(model, text, tab, "byte")
        seg_ids, seg_offs = S.encode_segments(model, text, tab)
        assert ids == seg_ids and offs == seg_offs, (k, text, vocab, listed)
        assert S.encode_special(model, text, tab, None) == (ids, None)
        lits = S.find(text, tab)
        n_literals += len(lits)
        # code points: every span is the byte span counted in valid code points in front of it
        cids, coffs = S.encode_special(model, text, tab, "char")
        pre = S._cp_before(text)
        assert cids == ids and [o[0] for o in coffs] == [pre[b] for b, _ in offs], (k, text)
        if not lits:
            assert (ids, offs) == tuple(model.encode_with_offsets(text, "byte"))
    assert n_literals >= 4000


def test_rows_are_the_documents_one_by_one():
    vocab = ["[UNK]", "[MASK]", "[SEP]", "a", "##b", "é"]
    model, tab = R.Model(vocab), S.table(vocab, [1, 2])
    docs = ["[MASK]", "", "ab [SEP]", "é[MASK]é", "[SEP][MASK]", "x"]
    ids, splits, offs = S.encode_special_rows(model, docs, tab, "char")
    assert ids == [1, 3, 4, 2, 5, 1, 5, 2, 1, 0] and splits == [0, 1, 1, 4, 7, 9, 10]
    assert offs == [(0, 6), (0, 1), (1, 2), (3, 8), (0, 1), (1, 7), (7, 8), (0, 5), (5, 11), (0, 1)]
    bids, _, boffs = S.encode_special_rows(model, docs, tab, "byte")
    assert bids == ids and boffs[4:7] == [(0, 2), (2, 8), (8, 10)]
    assert S.encode_special_rows(model, docs, tab) == (ids, splits, None)
