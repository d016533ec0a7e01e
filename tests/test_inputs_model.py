"""CPU checks of the model-inputs contract (tests/inputs_model.py): the invariants of plan() over a grid of lengths,
budgets and strides, the pinned examples of the longest_first rule, build() on a hand-made batch, and — where the
`tokenizers` package is present — the same grid against HF's fast tokenizer."""
import pytest

import inputs_model as I
import rows_model as R

LA = LB = range(21)
BUDGETS = range(17)
CLS, SEP, PAD = 1, 2, 0


def _spec(B, pairs, truncation, stride):
    return I.Spec(B + 1 + (2 if pairs else 1), CLS, SEP, PAD, pairs, truncation, stride)


def _grid():
    """every (la, lb, spec) of the grid that the argument rules let through, pairs and single sequences"""
    for B in BUDGETS:
        for stride in range(-1, max(B, 0)):
            for pairs, trunc in ((0, I.LONGEST_FIRST), (1, I.LONGEST_FIRST), (0, I.ONLY_FIRST), (1, I.ONLY_FIRST), (1, I.ONLY_SECOND)):
                if trunc == I.LONGEST_FIRST and stride >= 0:
                    continue
                spec = _spec(B, pairs, trunc, stride)
                if trunc != I.LONGEST_FIRST and B < max(stride, 0) + 1:
                    with pytest.raises(ValueError, match="no room for a window"):
                        I.plan(0, 0, spec)
                    continue
                for la in LA:
                    for lb in (LB if pairs else (0,)):
                        yield la, lb, spec


def test_plan_invariants():
    n = n_windowed = 0
    for la, lb, spec in _grid():
        B, st = I.budget(spec), max(spec.stride, 0)
        wins, cut = I.plan(la, lb, spec)
        label = (la, lb, spec)
        n += 1
        assert len(wins) >= 1, label
        for (a0, a1), (b0, b1) in wins:  # a row never exceeds max_len
            assert 0 <= a0 <= a1 <= la and 0 <= b0 <= b1 <= lb, label
            assert I.specials(spec) + (a1 - a0) + (b1 - b0) <= spec.max_len, label
        kept_a = set().union(*[range(*w[0]) for w in wins])
        kept_b = set().union(*[range(*w[1]) for w in wins])
        assert cut == (len(kept_a) < la or len(kept_b) < lb), label  # cut: ids that are in no row
        if spec.truncation == I.LONGEST_FIRST:
            (a, b), = wins
            assert a[0] == 0 and b[0] == 0 and a[1] + b[1] == min(la + lb, B), label
            if la + lb > B:  # neither side gives way below half the budget while the other is above it
                assert min(a[1], b[1]) >= min(la, lb, B // 2), label
            continue
        side = 0 if (not spec.pairs or spec.truncation == I.ONLY_FIRST) else 1
        l, lF = (la, lb) if side == 0 else (lb, la)
        fixed = [w[1 - side] for w in wins]
        kF = min(lF, B - st - 1) if spec.pairs else 0
        assert all(f == (0, kF) for f in fixed), label  # the fixed side is repeated in every window
        w = [x[side] for x in wins]
        W = B - kF
        if spec.stride < 0:  # window 0 only
            assert w == [(0, min(l, W))], label
            assert wins == I.plan(la, lb, spec._replace(stride=0))[0][:1], label
            continue
        assert set().union(*[range(*x) for x in w]) == set(range(l)), label  # every id of the windowed side is in a window
        assert w[0][0] == 0 and w[-1][1] == l, label
        for x, y in zip(w, w[1:]):  # neighbours overlap by exactly the stride; all windows but the last are full
            assert x[1] - y[0] == spec.stride and x[1] - x[0] == W and y[0] > x[0], label
        assert w[-1][1] - w[-1][0] <= W, label
        if len(w) > 1:
            assert w[-1][1] - w[-1][0] > spec.stride, label  # the last window holds an id that no other has
            n_windowed += 1
    assert n == sum(1 for _ in _grid())
    assert n > 100000 and n_windowed > 30000, (n, n_windowed)


def test_longest_first_pinned_examples():
    def keep(la, lb, B):
        (a, b), = I.plan(la, lb, _spec(B, 1, I.LONGEST_FIRST, -1))[0]
        return a[1], b[1]
    assert keep(5, 5, 7) == (3, 4)  # (HF's slow tokenizer gives (4, 3): the fast one is followed)
    assert keep(6, 5, 7) == (4, 3)
    assert keep(4, 10, 7) == (3, 4)
    assert keep(10, 4, 7) == (4, 3)
    assert keep(3, 3, 7) == (3, 3) and keep(0, 9, 4) == (0, 4) and keep(9, 0, 4) == (4, 0) and keep(9, 9, 0) == (0, 0)
    assert keep(1, 9, 6) == (1, 5) and keep(9, 1, 6) == (5, 1)
    (a, b), = I.plan(9, 0, I.Spec(6, CLS, SEP, PAD, 0, I.LONGEST_FIRST, -1))[0]
    assert (a, b) == ((0, 4), (0, 0))


def test_argument_rules():
    ok = I.Spec(8, CLS, SEP, PAD, 1, I.ONLY_FIRST, 2)
    I.check(ok, 4)
    for bad, msg in ((ok._replace(truncation=3), "truncation"), (ok._replace(stride=-2), "stride"), (ok._replace(pairs=2), "pairs"),
                     (ok._replace(max_len=0), "max_len"), (ok._replace(max_len=2), "max_len"),
                     (ok._replace(truncation=I.LONGEST_FIRST), "windows"), (ok._replace(pairs=0, truncation=I.ONLY_SECOND), "only_second"),
                     (ok._replace(stride=5), "no room"), (ok._replace(max_len=3, stride=-1), "no room")):
        with pytest.raises(ValueError, match=msg):
            I.check(bad, 4)
    with pytest.raises(ValueError, match="even number"):
        I.check(ok, 3)
    I.check(ok._replace(max_len=3, truncation=I.LONGEST_FIRST, stride=-1), 0)  # B == 0: rows of specials


VOCAB = ["[UNK]", "[CLS]", "[SEP]", "a", "b", "c", "d", "e", "##x"]


def test_build_by_hand():
    model = R.Model(VOCAB)
    docs = ["a b c d e", "b ax", "", "c"]  # ("ax" is a + ##x: two ids, spans (2, 3), (3, 4))
    out = I.build(model, docs, I.Spec(8, 1, 2, 9, 1, I.LONGEST_FIRST, -1), "char")
    assert out["input_ids"] == [[1, 3, 4, 5, 2, 4, 3, 2], [1, 2, 5, 2, 9, 9, 9, 9]]
    assert out["token_type_ids"] == [[0, 0, 0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 0, 0, 0, 0]]
    assert out["lengths"] == [8, 4] and out["sample"] == [0, 1] and (out["n_cut"], out["n_windowed"]) == (1, 0)
    assert out["offsets"][0] == [(0, 0), (0, 1), (2, 3), (4, 5), (0, 0), (0, 1), (2, 3), (0, 0)]
    assert out["offsets"][1] == [(0, 0), (0, 0), (0, 1), (0, 0)] + [(0, 0)] * 4
    out = I.build(model, docs, I.Spec(7, 1, 2, 9, 1, I.ONLY_FIRST, 1), "byte")  # B = 4, kF = min(lb, 2), W = 2 / 3, step = 1 / 2
    assert out["input_ids"] == [[1, 3, 4, 2, 4, 3, 2], [1, 4, 5, 2, 4, 3, 2], [1, 5, 6, 2, 4, 3, 2], [1, 6, 7, 2, 4, 3, 2],
                                [1, 2, 5, 2, 9, 9, 9]]
    assert out["sample"] == [0, 0, 0, 0, 1] and out["lengths"] == [7, 7, 7, 7, 4] and (out["n_cut"], out["n_windowed"]) == (1, 1)
    assert out["offsets"][3] == [(0, 0), (6, 7), (8, 9), (0, 0), (0, 1), (2, 3), (0, 0)]
    out = I.build(model, docs, I.Spec(3, None, None, 9, 0, I.ONLY_FIRST, 0))
    assert out["input_ids"] == [[3, 4, 5], [6, 7, 9], [4, 3, 8], [9, 9, 9], [5, 9, 9]] and out["sample"] == [0, 0, 1, 2, 3]
    assert out["token_type_ids"] == [[0] * 3] * 5 and out["offsets"] is None and out["n_windowed"] == 1 and out["n_cut"] == 0
    with pytest.raises(ValueError, match="even number"):
        I.build(model, docs[:3], I.Spec(8, 1, 2, 9, 1))


def test_against_hf_fast_tokenizer():
    """an extra: the grid against tokenizers' truncation, for the three strategies, and its overflowing encodings for
    the windows (where the fixed side fits: HF raises where it does not); ids, type ids and offsets"""
    tk = pytest.importorskip("tokenizers")
    words_a = ["a%02d" % i for i in range(len(LA))]
    words_b = ["b%02d" % i for i in range(len(LB))]
    vocab = {"[UNK]": 0, "[CLS]": CLS, "[SEP]": SEP}
    vocab.update({w: 10 + i for i, w in enumerate(words_a)})
    vocab.update({w: 100 + i for i, w in enumerate(words_b)})
    tok = tk.Tokenizer(tk.models.WordLevel(vocab, unk_token="[UNK]"))
    tok.pre_tokenizer = tk.pre_tokenizers.WhitespaceSplit()
    tok.post_processor = tk.processors.TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1",
                                                          special_tokens=[("[CLS]", CLS), ("[SEP]", SEP)])
    names = {I.LONGEST_FIRST: "longest_first", I.ONLY_FIRST: "only_first", I.ONLY_SECOND: "only_second"}
    n = n_windows = 0
    last = None
    for la, lb, spec in _grid():
        B, st = I.budget(spec), max(spec.stride, 0)
        if spec.truncation != I.LONGEST_FIRST and spec.pairs and (lb if spec.truncation == I.ONLY_FIRST else la) > B - st - 1:
            continue  # (the fixed side does not fit)
        if spec != last:
            tok.enable_truncation(spec.max_len, stride=st, strategy=names[spec.truncation])
            last = spec
        ta, tb = " ".join(words_a[:la]), " ".join(words_b[:lb])
        enc = tok.encode(ta, tb) if spec.pairs else tok.encode(ta)
        encs = [enc] + (list(enc.overflowing) if spec.stride >= 0 else [])
        wins, _ = I.plan(la, lb, spec)
        assert len(encs) == len(wins), (la, lb, spec)
        for e, ((a0, a1), (b0, b1)) in zip(encs, wins):
            ids = [CLS] + list(range(10 + a0, 10 + a1)) + [SEP]
            types = [0] * len(ids)
            offs = [(0, 0)] + [(4 * i, 4 * i + 3) for i in range(a0, a1)] + [(0, 0)]
            if spec.pairs:
                ids += list(range(100 + b0, 100 + b1)) + [SEP]
                types += [1] * (b1 - b0 + 1)
                offs += [(4 * i, 4 * i + 3) for i in range(b0, b1)] + [(0, 0)]
            assert e.ids == ids and e.type_ids == types and e.offsets == offs, (la, lb, spec, e.ids, ids)
        n += 1
        n_windows += len(wins) > 1
    assert (n, n_windows) == (51030, 19992)  # (the grid is fixed: no case may drop out silently)
