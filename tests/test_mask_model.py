"""The masking model (tests/mask_model.py) against known answers of the draw, hand-written cases, its properties over
random batches, the binomial bounds of the selection and of the mask / random / keep split, and — when the `tokenizers`
package is present — HF's Encoding.word_ids."""
import math
import random

import pytest

import mask_model as M

LETTERS = "abcdefghijklmnopqrstuvwxyz"
# [UNK] [CLS] [SEP] [PAD] [MASK], words, continuations, one malformed line
VOCAB = ["[UNK]", "[CLS]", "[SEP]", "[PAD]", "[MASK]", "un", "##aff", "##able", ",", "x", "##y", "z", ".."] + \
        list(LETTERS[:8]) + ["##" + ch for ch in LETTERS[:8]]
ID = {t: i for i, t in enumerate(VOCAB)}
FLAGS = M.flags_of(VOCAB)
CLS, SEP, PAD, MASK = ID["[CLS]"], ID["[SEP]"], ID["[PAD]"], ID["[MASK]"]
SPEC = M.Spec(max_len=0, cls_id=CLS, sep_id=SEP, pad_id=PAD, mask_id=MASK)


def _ids(text):
    return [ID[t] for t in text.split()]


def test_draw_known_answers():
    assert M.draw(0, 0, 0, 0) == 2802244911
    assert M.draw(0, 0, 0, 1) == 3011683077
    assert M.draw(1, 2, 3, 2) == 4227405288
    assert M.draw(2 ** 64 - 1, 2 ** 40, 511, 0) == 1078768590
    assert M.draw(12345, 7, 64, 1) == 1139674002
    # the vectorised form the transform uses is the same function
    for seed, row, stream in ((0, 0, 0), (1, 2, 2), (2 ** 64 - 1, 2 ** 40, 0), (12345, 7, 1)):
        assert M.draw_row(seed, row, 600, stream) == [M.draw(seed, row, c, stream) for c in range(600)]
    assert M.q32(0.0) == 0 and M.q32(1.0) == 2 ** 32 and M.q32(0.5) == 2 ** 31 and M.q32(0.15) == int(0.15 * 2 ** 32)


def test_flags_follow_the_library():
    """the model's classification of the test vocabularies is wp_vocab_token_flags (needs no device)"""
    import wordpiece_amd as W
    from test_gpu_mask import VOCAB as GPU_VOCAB
    for lines in (VOCAB, GPU_VOCAB):
        v = W.Vocab(lines)
        assert [v.token_flags(i) for i in range(len(lines))] == M.flags_of(lines)
    assert FLAGS[ID["[UNK]"]] == 3 and FLAGS[ID[".."]] == 5 and FLAGS[ID["##y"]] == 0 and FLAGS[ID["x"]] == 1


def test_hand_written_word_ids():
    row = _ids("[CLS] un ##aff ##able , x [SEP] ##y z [SEP] [PAD]")
    assert M.word_ids(FLAGS, [row], None, SPEC) == [[-1, 0, 0, 0, 1, 2, -1, 0, 1, -1, -1]]
    # the same through lengths instead of a pad id
    spec = SPEC._replace(pad_id=-1)
    assert M.word_ids(FLAGS, [row], [10], spec) == [[-1, 0, 0, 0, 1, 2, -1, 0, 1, -1, -1]]
    assert M.word_ids(FLAGS, [row], None, spec)[0][-1] == 0  # ([PAD] without a pad id: a special, a word of its own behind the [SEP])
    # an [UNK] followed by a ## token: two words
    out, solo, start, wid, w = M.structure(FLAGS, _ids("[UNK] ##y"), None, SPEC)
    assert solo == [True, False] and start == [True, True] and wid == [0, 1] and w == [0, 1]
    out, solo, start, wid, w = M.structure(FLAGS, _ids("x .. ##y ##y"), None, SPEC)  # a malformed token is solo too
    assert solo == [False, True, False, False] and start == [True, True, True, False] and wid == [0, 1, 2, 2] and w == [0, 1, 2, 2]
    # a row that begins with ##: starts a word
    out, solo, start, wid, w = M.structure(FLAGS, _ids("##aff ##able x ##y"), None, SPEC)
    assert start == [True, False, True, False] and wid == [0, 0, 1, 1] and w == [0, 0, 2, 2]
    # ids outside the vocabulary are outside, lengths are clamped
    assert M.word_ids(FLAGS, [[-1, ID["##y"], len(VOCAB), ID["x"], 2 ** 31 - 1]], None, SPEC) == [[-1, 0, -1, 0, -1]]
    assert M.word_ids(FLAGS, [[ID["x"]] * 3] * 3, [-5, 2, 99], SPEC) == [[-1, -1, -1], [0, 1, -1], [0, 1, 2]]


def test_hand_written_transform():
    row = _ids("[CLS] un ##aff ##able , [UNK] x [SEP] [PAD]")
    spec = SPEC._replace(select_q32=M.ONE, mask_q32=M.ONE)
    res = M.mask(FLAGS, [row], None, spec)
    assert res["input_ids"] == [[CLS, MASK, MASK, MASK, MASK, ID["[UNK]"], MASK, SEP, PAD]]
    assert res["labels"] == [[-100] + row[1:5] + [-100, ID["x"], -100, -100]]
    assert res["stats"] == dict(n_rows=1, n_words=4, n_selected=5, n_selected_units=3, n_masked=5, n_random=0, n_kept=0, whole_word=1)
    res = M.mask(FLAGS, [row], None, spec._replace(whole_word=0, mask_q32=0, random_q32=M.ONE, seed=3, row_base=5))
    assert res["stats"] == dict(n_rows=1, n_words=4, n_selected=5, n_selected_units=5, n_masked=0, n_random=5, n_kept=0, whole_word=0)
    assert [res["input_ids"][0][c] for c in (1, 2, 3, 4, 6)] == [(M.draw(3, 5, c, 2) * len(VOCAB)) >> 32 for c in (1, 2, 3, 4, 6)]


def random_batch(rng, n_rows, max_len, vocab_size, flags, specials=(1, 2, 3)):
    """ids with about half continuations, some [UNK], ids out of range and specials in odd places; lengths or None"""
    cont = [i for i in range(vocab_size) if flags[i] == 0]
    init = [i for i in range(vocab_size) if flags[i] == 1]
    odd = [i for i in range(vocab_size) if flags[i] & 6 and i not in specials]
    ids = []
    for _ in range(n_rows):
        row = []
        for _ in range(max_len):
            k = rng.random()
            if k < 0.46:
                row.append(rng.choice(cont))
            elif k < 0.88:
                row.append(rng.choice(init))
            elif k < 0.92:
                row.append(rng.choice(odd))
            elif k < 0.95:
                row.append(rng.choice((-1, vocab_size, 2 ** 31 - 1, -2 ** 31)))
            else:
                row.append(rng.choice(specials))
        ids.append(row)
    lengths = None if rng.random() < 0.3 else [rng.choice((0, max_len, rng.randint(0, max_len), max_len + 3, -1)) for _ in range(n_rows)]
    return ids, lengths


def test_properties_over_random_batches():
    rng = random.Random(11)
    n_whole = 0
    for trial in range(60):
        n_rows, max_len = rng.randint(1, 9), rng.choice((1, 2, 5, 17, 40))
        ids, lengths = random_batch(rng, n_rows, max_len, len(VOCAB), FLAGS, (CLS, SEP, PAD))
        spec = SPEC._replace(max_len=max_len, whole_word=trial & 1, select_q32=M.q32(rng.choice((0.15, 0.5, 0.9))), mask_q32=M.q32(0.8),
                             random_q32=M.q32(0.1), seed=rng.getrandbits(64), row_base=rng.choice((0, 7, 2 ** 63)), ignore_id=-7)
        res = M.mask(FLAGS, ids, lengths, spec)
        st = res["stats"]
        assert st["n_masked"] + st["n_random"] + st["n_kept"] == st["n_selected"] == sum(map(sum, res["selected"]))
        assert st["n_selected_units"] <= st["n_selected"] and (spec.whole_word or st["n_selected_units"] == st["n_selected"])
        for r, row in enumerate(ids):
            outside, solo, start, wid, w = M.structure(FLAGS, row, None if lengths is None else lengths[r], spec)
            sel = res["selected"][r]
            for c, x in enumerate(row):
                assert (res["labels"][r][c] != spec.ignore_id) == sel[c] and (not sel[c] or res["labels"][r][c] == x)
                assert sel[c] or res["input_ids"][r][c] == x
                assert not (sel[c] and (outside[c] or solo[c]))
                if spec.whole_word and not outside[c]:
                    assert sel[c] == sel[w[c]] and wid[c] == wid[w[c]]  # the tokens of a word: all or none
                    n_whole += c != w[c]
        # nothing and everything
        none = M.mask(FLAGS, ids, lengths, spec._replace(select_q32=0))
        assert none["input_ids"] == [[int(x) for x in row] for row in ids] and none["stats"]["n_selected"] == 0
        assert all(lab == spec.ignore_id for row in none["labels"] for lab in row)
        full = M.mask(FLAGS, ids, lengths, spec._replace(select_q32=M.ONE, mask_q32=M.ONE, random_q32=0))
        for r, row in enumerate(ids):
            outside, solo, _, _, _ = M.structure(FLAGS, row, None if lengths is None else lengths[r], spec)
            assert full["selected"][r] == [not o and not s for o, s in zip(outside, solo)]
            assert all(y == MASK for y, s in zip(full["input_ids"][r], full["selected"][r]) if s)
        assert full["stats"]["n_masked"] == full["stats"]["n_selected"]
        # rows [a, b) with row_base + a are the slice of the whole batch
        a = rng.randint(0, n_rows - 1)
        b = rng.randint(a, n_rows)
        part = M.mask(FLAGS, ids[a:b], None if lengths is None else lengths[a:b], spec._replace(row_base=(spec.row_base + a) & M.M64))
        for key in ("input_ids", "labels", "word_ids"):
            assert part[key] == res[key][a:b]
    assert n_whole > 300


P_CASES = [(p, seed) for p in (0.01, 0.15, 0.5) for seed in range(40)]


def _within(n, N, p):
    return abs(n - N * p) <= 4 * math.sqrt(N * p * (1 - p))


def test_selected_share_and_split_lie_within_four_sigma():
    """64 x 128 all-selectable cells, whole_word = 0: |n - Np| <= 4 sqrt(N p (1 - p)) for the selected cells, and for the
    mask / random / keep split of the selected ones (p: the q32 over 2^32)"""
    rows = [[ID["x"]] * 128] * 64
    N = 64 * 128
    worst = 0.0
    for p, seed in P_CASES:
        spec = SPEC._replace(max_len=128, whole_word=0, select_q32=M.q32(p), mask_q32=M.q32(0.8), random_q32=M.q32(0.1), seed=seed)
        st = M.mask(FLAGS, rows, None, spec)["stats"]
        ps = spec.select_q32 / 2 ** 32
        worst = max(worst, abs(st["n_selected"] - N * ps) / math.sqrt(N * ps * (1 - ps)))
        assert _within(st["n_selected"], N, ps), (p, seed, st)
        n = st["n_selected"]
        pm, pr = spec.mask_q32 / 2 ** 32, spec.random_q32 / 2 ** 32
        assert _within(st["n_masked"], n, pm) and _within(st["n_random"], n, pr) and _within(st["n_kept"], n, 1 - pm - pr), (p, seed, st)
    print("worst |z| of the selection: %.2f" % worst)


def test_word_ids_against_hf_tokenizers():
    tk = pytest.importorskip("tokenizers")
    vocab = {t: i for i, t in enumerate(VOCAB)}
    tok = tk.Tokenizer(tk.models.WordPiece(vocab, unk_token="[UNK]"))
    tok.pre_tokenizer = tk.pre_tokenizers.WhitespaceSplit()
    tok.post_processor = tk.processors.TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1",
                                                          special_tokens=[("[CLS]", CLS), ("[SEP]", SEP)])
    tok.enable_padding(length=16, pad_id=PAD, pad_token="[PAD]")
    rng = random.Random(5)
    words = ["unaffable", "unable", "x", "xy", "xyy", "z", ",", "abc", "hgfedcba", "qqq", "a", "ba", "unq"]
    n = 0
    for trial in range(120):
        a = " ".join(rng.choice(words) for _ in range(rng.randint(0, 4)))
        b = " ".join(rng.choice(words) for _ in range(rng.randint(0, 4))) if trial & 1 else None
        enc = tok.encode(a, b) if b is not None else tok.encode(a)
        if len(enc.ids) != 16:
            continue
        exp = [-1 if w is None else w for w in enc.word_ids]
        assert M.word_ids(FLAGS, [enc.ids], None, SPEC) == [exp], (a, b, enc.tokens)
        assert M.word_ids(FLAGS, [enc.ids], [sum(enc.attention_mask)], SPEC._replace(pad_id=-1)) == [exp], (a, b)
        n += 1
    assert n > 100
