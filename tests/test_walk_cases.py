"""CPU tests of the inputs behind test_gpu_walk_edges.py (walk_cases.py): the model of the class rule reproduces what every
builder of groups W to C claims to have built (stretch lengths, the gap, stretches above kWideMin, long words, ids), and the
references agree with each other on exactly these inputs: the oracle's ids with offsets_model.encode_spans, the oracle's
fast ids with the Python model of test_oracle_fast.py."""
import collections

import numpy as np
import pytest

import offsets_model as OM
import oracle_lib as O
import walk_cases as K
from test_oracle_fast import fast_model


def test_constants_are_read_from_the_headers():
    assert (K.WIDE_MIN, K.WIDE_PER_LANE, K.MAX_GAP, K.STAGE_IDS, K.WB_PER_WAVE, K.ANCHOR_BYTES, K.BLOCK, K.WAVE) == \
        (48, 4, 2048, 4, 256, 16, 256, 64), "a constant of the walk changed: the cases moved with it — check GROUP_SIZES and update this line"


def test_case_count_per_group():
    count = collections.Counter(n[0] for n in K.CASES)
    assert {g: count[g] for g in "WLSBAC"} == K.GROUP_SIZES
    assert count["F"] == K.F_SEEDS == 200
    assert set(count) == set(K.GROUPS)
    assert all(n in K.CASES for n in K.EMBEDDED) and {n[0] for n in K.EMBEDDED} == set("WLSBAC")


def test_model_on_hand_made_texts():
    """the model itself, on texts small enough to check by eye"""
    m = K.Model("ab, cd  中e", K.single())
    assert m.all_hard and m.linear_anchors() == [0, 2, 4, 8, 9] and m.fast_anchors() == [0, 2, 4, 8]
    assert m.linear()["max_anchor_gap"] == 4 and m.stretches(m.linear_anchors())[-2:] == [(8, 9), (9, 10)]
    m = K.Model("  a b.c,d", K.soft())
    assert not m.all_hard and m.soft == {32, 44, 0x4e2d, 0x6587}
    assert m.linear_anchors() == [5, 6] and m.linear()["max_anchor_gap"] == 5   # only '.' is hard: itself and what follows it
    assert m.fast_anchors() == [2, 4, 5, 6, 7, 8]
    m = K.Model("x" * 3000 + " " * 5000 + "y", K.single())
    assert m.linear()["max_anchor_gap"] == K.MAX_GAP + 1 and m.linear()["n_long_words"] == 1 and m.linear()["anchor_mode"] == 2
    m = K.Model("x" * 2048 + " " * 5000 + "y", K.single())
    assert m.linear() == dict(anchor_mode=0, staged_emit=1, lean=1, n_wide_words=1, n_long_words=0, max_anchor_gap=2048, n_anchors=2)


@pytest.mark.parametrize("name", K.names())
def test_case_is_what_its_builder_claims(name):
    text, vocab, expect = K.build(name)
    claims = dict(expect["claims"])
    assert claims, "a case of groups W to C states its branch"
    m = expect["model"]
    ov = O.Vocab(vocab)
    ids = ov.encode(text).tolist()
    n_ids = claims.pop("n_ids", None)
    if n_ids is not None:
        assert len(ids) == n_ids, (len(ids), n_ids)
    longest = claims.pop("longest", None)
    if longest is not None:
        assert max(hi - lo for lo, hi in m.stretches(m.linear_anchors())) == longest
    for key, want in claims.items():
        side, field = key.split("_", 1)
        got = expect[{"lin": "linear", "fast": "fast"}[side]]
        assert got is not None and got[field] == want, (key, got, want)
    # two references against each other
    ids2, spans, t, starts = OM.encode_spans(text, vocab)
    assert ids2 == ids
    OM.check_coverage(text, ids2, spans, t, starts)
    if expect["fast"] is not None:
        assert ov.fast_encode(text).tolist() == fast_model(text, vocab)


@pytest.mark.parametrize("block", range(8))
def test_composed_cases_agree_between_references(block):
    for name in K.names("F")[block::8]:
        text, vocab, expect = K.build(name)
        assert len(text) > 0
        ov = O.Vocab(vocab)
        ids2, spans, t, starts = OM.encode_spans(text, vocab)
        assert ids2 == ov.encode(text).tolist(), name
        if expect["fast"] is not None:
            assert ov.fast_encode(text).tolist() == fast_model(text, vocab), name


def test_composed_cases_reach_every_branch():
    """group F is compared without branch assertions; the seeds between them still reach every variant"""
    seen = collections.Counter()
    for name in K.names("F"):
        lin = K.build(name)[2]["linear"]
        seen[(lin["anchor_mode"], lin["lean"], lin["n_wide_words"] > 0)] += 1
    assert {(0, 1, False), (0, 1, True), (2, 0, False), (1, 1, False), (0, 0, False)} <= set(seen), seen
