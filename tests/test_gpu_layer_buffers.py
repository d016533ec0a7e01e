"""GPU tests (-m gpu) of the device buffers of the layers on top of the encoder (csrc/rows_path.h, inputs_path.h,
mask_path.h, detok_path.h, pack_path.h, the pre-pass of csrc/normalize.h, and the grouping layers: count_path.h,
learn_path.h, dedup_path.h, neardup_path.h over group_path.h, overlap_path.h and repeat_path.h over window_path.h) across
the calls of one handle.  Every layer lays its buffers out with an Arena over a DeviceBuffer that grows when a call needs
more than it holds, and two mistakes
show only from one call to the next: a sequence of allocations that differs between the planning pass and the real one,
and a pointer kept across a regrowth.  So every layer is called small, then large enough to make its buffers grow, then
small again, all on ONE handle (the per-document route needs a vocabulary of its own, hence a second handle for it alone),
and every result is compared exactly with the Python models.

A DeviceBuffer keeps bytes / 16 + 1 MiB of slack: a layer's sequence starts from released buffers (Vocab.trim()), the
small call allocates about 1 MiB and the large one needs GROW bytes or more (asserted case by case).  The small cases
hold 31 rows and 64 ids: 32 row_splits and 64 ids are 256 bytes each, where the arena's rounding to 256 bytes adds
nothing behind an array; 8 rows is the other small size."""
import random

import numpy as np
import pytest

import count_model as CM
import dedup_model as DDM
import detok_model as DM
import inputs_model as I
import learn_model as LM
import mask_model as MM
import neardup_model as NDM
import normalize_model as NM
import overlap_model as OM
import pack_model as PM
import repeat_model as RM
import rows_model as R
import wordpiece_amd as W

LETTERS = "abcdefghijklmnopqrstuvwxyz"
VOCAB = ["[UNK]", "[CLS]", "[SEP]", "[PAD]", "[MASK]"] + list(LETTERS) + ["##" + ch for ch in LETTERS] + ["é", "##é"]
CLS, SEP, PAD, MASK = 1, 2, 3, 4
NEWLINE_VOCAB = VOCAB + ["a\nb"]  # an eligible token with U+000A: every documents call goes document by document
GROW = (1 << 20) + (1 << 16)  # more than the 1 MiB of slack and the sixteenth of a small call's bytes


class Memo:
    """rows_model.Model behind a cache by document: the batches below repeat the documents of a small pool"""

    def __init__(self, vocab):
        self.model, self.seen = R.Model(vocab), {}

    def encode_with_offsets(self, text, unit="byte"):
        key = (bytes(text), unit)
        if key not in self.seen:
            self.seen[key] = self.model.encode_with_offsets(text, unit)
        return self.seen[key]


def _word(rng):
    return "".join(rng.choice(LETTERS) for _ in range(rng.choice((1, 1, 2, 3))))


def _doc(rng, n_words):
    return " ".join(_word(rng) for _ in range(n_words)).encode()


def _pool():
    rng = random.Random(7)
    return [b""] + [_doc(rng, n) for n in (1, 2, 3, 5, 8, 13) for _ in range(8)]


@pytest.fixture(scope="module")
def gv():
    return W.Vocab(VOCAB)


@pytest.fixture(scope="module")
def model():
    return Memo(VOCAB)


POOL = _pool()


def docs_of(n, seed, short=False):
    rng = random.Random(seed)
    pool = POOL[:25] if short else POOL  # short: documents of at most three words
    return [rng.choice(pool) for _ in range(n)]


def docs_with_ids(model, n_docs, n_ids, seed):
    """n_docs documents with n_ids ids between them"""
    rng = random.Random(seed)
    docs, left = [], n_ids
    for _ in range(n_docs - 1):
        d = rng.choice(POOL[:17])
        n = len(model.encode_with_offsets(d)[0])
        docs.append(d if n <= left else b"")
        left -= n if n <= left else 0
    return docs + [" ".join(LETTERS[k % 26] for k in range(left)).encode()]  # one-letter words: an id each


def small_then_large(gv, run, small31, large, small8):
    """one layer's sequence from released buffers: small (256-byte arrays), large (the buffers grow), small, small"""
    gv.trim()
    for case in (small31, large, small8, small31):
        run(case)


def _rows_equal(got, exp, unit):
    assert np.array_equal(got[0], np.array(exp[0], dtype=np.int32))
    assert np.array_equal(got[1], np.array(exp[1], dtype=np.int64))
    if unit:
        assert np.array_equal(got[2], np.array(exp[2], dtype=np.uint32).reshape(-1, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("unit", [None, "byte"])
def test_rows_explicit_and_lines(gv, model, unit):
    def run(docs):
        text, starts = R.join_docs(docs)
        exp = R.encode_rows(model, docs, unit)
        _rows_equal(gv.encode_rows(text=text, doc_offsets=starts, offsets=unit), exp, unit)
        lines = R.split_lines(text)
        _rows_equal(gv.encode_rows(text=text, offsets=unit), R.encode_rows(model, lines, unit), unit)
        assert gv.stats()["rows_route"] == 1 and gv.stats()["n_rows"] == len(lines)

    n_large = 150000
    assert (n_large + 1) * 8 > GROW  # the explicit row starts in rows_in
    small_then_large(gv, run, docs_with_ids(model, 31, 64, 1), docs_of(n_large, 2, short=True), docs_of(8, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("unit", [None, "char"])
def test_rows_document_by_document(unit):
    gv, model = W.Vocab(NEWLINE_VOCAB), Memo(NEWLINE_VOCAB)
    rng = random.Random(11)
    big = [_doc(rng, 40000), _doc(rng, 30000)]

    def run(docs):
        text, starts = R.join_docs(docs)
        exp = R.encode_rows(model, docs, unit)
        _rows_equal(gv.encode_rows(text=text, doc_offsets=starts, offsets=unit), exp, unit)
        assert gv.stats()["rows_route"] == 0
        lines = R.split_lines(text)
        _rows_equal(gv.encode_rows(text=text, offsets=unit), R.encode_rows(model, lines, unit), unit)
        assert gv.stats()["rows_route"] == 0 and gv.stats()["n_rows"] == len(lines)

    large = [big[0], b"", big[1], big[0], POOL[5], big[1], big[0], big[1]]
    assert 4 * sum(len(model.encode_with_offsets(d)[0]) for d in large) > GROW  # the ids of the result block in rows_out
    small_then_large(gv, run, docs_with_ids(model, 31, 64, 12), large, docs_of(8, 13))


@pytest.mark.gpu
def test_padded(gv, model):
    L = 16

    def run(docs):
        text, starts = R.join_docs(docs)
        ids, splits, _ = R.encode_rows(model, docs)
        rows, lengths, cut = R.pack(ids, splits, L, CLS, SEP, PAD)
        got = gv.encode_padded(text=text, doc_offsets=starts, max_len=L, cls_id=CLS, sep_id=SEP, pad_id=PAD)
        assert np.array_equal(got[0], np.array(rows, dtype=np.int32).reshape(len(docs), L))
        assert np.array_equal(got[1], np.array(lengths, dtype=np.int32))
        assert gv.stats()["rows_truncated"] == cut

    n_large = 40000
    assert n_large * L * 4 > GROW  # the batch in pad_buf
    small_then_large(gv, run, docs_with_ids(model, 31, 64, 21), docs_of(n_large, 22), docs_of(8, 23))


@pytest.mark.gpu
@pytest.mark.parametrize("windows", [False, True])
def test_inputs(gv, model, windows):
    spec = I.Spec(8, CLS, SEP, PAD, 0, I.ONLY_FIRST, 2) if windows else I.Spec(16, CLS, SEP, PAD, 1, I.LONGEST_FIRST, -1)
    unit = "byte" if windows else None

    def run(docs):
        text, starts = R.join_docs(docs)
        exp = I.build(model, docs, spec, unit)
        got = gv.encode_inputs(text=text, doc_offsets=starts, pairs=bool(spec.pairs), max_len=spec.max_len, cls_id=CLS, sep_id=SEP,
                               pad_id=PAD, truncation="only_first" if windows else "longest_first", stride=2 if windows else None,
                               offsets=unit)
        n = len(exp["lengths"])
        for k in ("input_ids", "token_type_ids"):
            assert np.array_equal(got[k], np.array(exp[k], dtype=np.int32).reshape(n, spec.max_len)), k
        for k in ("lengths", "sample"):
            assert np.array_equal(got[k], np.array(exp[k], dtype=np.int32)), k
        if unit:
            assert np.array_equal(got["offsets"], np.array(exp["offsets"], dtype=np.uint32).reshape(n, spec.max_len, 2))
        ist = gv.inputs_stats()
        assert (ist["n_samples"], ist["n_out"], ist["n_cut"], ist["n_windowed"]) == (exp["n_samples"], n, exp["n_cut"], exp["n_windowed"])

    n_large = 60000 * (2 if spec.pairs else 1)
    assert 60000 * (16 + 4) > GROW  # a record and a window count per sample in inputs_buf; the batch in pad_buf is larger
    small_then_large(gv, run, docs_with_ids(model, 32 if spec.pairs else 31, 64, 31), docs_of(n_large, 32), docs_of(8, 33))


def _mask_rows(n_rows, max_len, seed):
    """rows drawn from 64 random ones (test_mask_model.random_batch), with lengths"""
    from test_mask_model import random_batch
    rng = random.Random(seed)
    flags = MM.flags_of(VOCAB)
    base, _ = random_batch(rng, 64, max_len, len(VOCAB), flags, (CLS, SEP, PAD))
    pick = np.array([rng.randrange(64) for _ in range(n_rows)])
    ids = np.array(base, dtype=np.int64).astype(np.int32)[pick]
    lengths = np.array([rng.choice((max_len, max_len, rng.randint(0, max_len))) for _ in range(n_rows)], dtype=np.int32)
    return ids, lengths


@pytest.mark.gpu
def test_mask_and_word_ids(gv):
    L = 16
    flags = MM.flags_of(VOCAB)
    assert [gv.token_flags(i) for i in range(len(VOCAB))] == flags
    spec = MM.Spec(L, CLS, SEP, PAD, MASK, -100, 1, MM.q32(0.3), MM.q32(0.8), MM.q32(0.1), 5, 0)
    kw = dict(mask_id=MASK, prob=0.3, mask_share=0.8, random_share=0.1, whole_word=True, seed=5, cls_id=CLS, sep_id=SEP, pad_id=PAD)

    def run(case):
        ids, lengths = case
        exp = MM.mask(flags, ids.tolist(), lengths.tolist(), spec)
        as2d = lambda rows: np.array(rows, dtype=np.int64).astype(np.int32).reshape(ids.shape)
        assert np.array_equal(gv.word_ids(ids, lengths, cls_id=CLS, sep_id=SEP, pad_id=PAD), as2d(exp["word_ids"]))
        for word_ids in (False, True):
            got = gv.mask_inputs(ids, lengths, word_ids=word_ids, **kw)
            assert sorted(got) == sorted(["input_ids", "labels"] + (["word_ids"] if word_ids else []))
            for k in got:
                assert np.array_equal(got[k], as2d(exp[k])), (k, word_ids)
            assert gv.mask_stats() == exp["stats"]

    n_large = 10000
    assert n_large * L * 4 * 2 > GROW  # ids and word ids in pad_buf, the smallest of the three forms
    small_then_large(gv, run, _mask_rows(31, L, 41), _mask_rows(n_large, L, 42), _mask_rows(8, L, 43))


def _cells(n_rows, per_row, seed):
    """ragged rows of ids of the vocabulary, some skipped, some outside it: (ids, row_splits); per_row 0: 64 ids over the rows"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 2 * per_row + 1, n_rows) if per_row else rng.multinomial(64, [1.0 / n_rows] * n_rows)
    splits = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(lens, out=splits[1:])
    ids = rng.integers(-1, len(VOCAB) + 1, int(splits[-1])).astype(np.int32)
    return ids, splits


@pytest.mark.gpu
def test_detokenize_ragged(gv):
    m = DM.Model.from_vocab(gv)

    def run(case):
        ids, splits = case
        for term in (None, "\n"):
            text, off = gv.detokenize(ids, row_splits=splits, skip_ids=[PAD, SEP], terminator=term, raw=True)
            exp_text, exp_off, exp_stats = m.detokenize_np(ids, splits, skip_ids=[PAD, SEP], terminator=term)
            assert np.array_equal(off, exp_off) and text == exp_text.tobytes()
            assert gv.detok_stats() == exp_stats

    large = _cells(60000, 12, 52)
    n_bytes = m.detokenize_np(large[0], large[1], skip_ids=[PAD, SEP])[2]["n_bytes"]
    assert 4 * len(large[0]) > GROW and 8 * len(large[1]) + n_bytes > GROW  # ids in detok_in; text_off and text in detok_out
    small = _cells(31, 0, 51)
    assert len(small[0]) == 64 and len(small[1]) == 32
    text, off = gv.detokenize(small[0], row_splits=small[1], raw=True)  # (the two forms of the model agree)
    assert (text, off.tolist()) == m.detokenize(small[0], row_splits=small[1])[:2]
    small_then_large(gv, run, small, large, _cells(8, 4, 53))


@pytest.mark.gpu
def test_detokenize_padded(gv):
    m = DM.Model.from_vocab(gv)
    L = 16

    def run(case):
        ids, lengths = case
        for lens in (lengths, None):
            text, off = gv.detokenize(ids, lengths=lens, skip_ids=[PAD], terminator=0, raw=True)
            exp_text, exp_off, exp_stats = m.detokenize(ids, lengths=lens, skip_ids=[PAD], terminator=0)
            assert off.tolist() == exp_off and text == exp_text
            assert gv.detok_stats() == exp_stats

    n_large = 20000
    assert n_large * L * 4 > GROW  # ids in detok_in
    small_then_large(gv, run, _mask_rows(31, L, 61), _mask_rows(n_large, L, 62), _mask_rows(8, L, 63))


@pytest.mark.gpu
@pytest.mark.parametrize("mode,want", [("next_fit", 0), ("next_fit", 7), ("stream", 0), ("stream", 7)])
def test_pack(gv, mode, want):
    L = 16

    def run(case):
        ids, splits = case
        ids = np.maximum(ids, 0)
        exp = PM.pack(ids, splits, L, PM.MODES[mode], CLS, SEP, PAD, PM.LONG_SPLIT, want)
        got = gv.pack_sequences(ids, splits, max_len=L, mode=mode, bos_id=CLS, eos_id=SEP, pad_id=PAD, long_docs="split", want=want)
        keys = ["input_ids", "lengths"] + (["segment_ids", "position_ids", "source"] if want else [])
        assert sorted(got) == sorted(keys)
        assert got["input_ids"].shape == (exp["n_out"], L)
        for k in keys:
            assert np.array_equal(got[k], exp[k]), k
        assert gv.pack_stats() == exp["stats"]

    large = _cells(150000, 2, 72)
    n_docs = len(large[1]) - 1
    # pieces and cells per document in pack_plan; the ids in pack_in; 24 bytes per piece in pack_tab; the batch in pack_out
    assert 8 * n_docs > GROW and 4 * len(large[0]) > GROW and 24 * np.count_nonzero(np.diff(large[1])) > GROW
    small_then_large(gv, run, _cells(31, 0, 71), large, _cells(8, 4, 73))


@pytest.mark.gpu
def test_normalising_handle_offsets(gv):
    flags = W.WP_NORM_BERT_UNCASED
    rng = random.Random(81)
    words = [_word(rng) for _ in range(40)] + ["É", "Ab", "ç", "x́"]

    def run(n_words):
        text = " ".join(rng.choice(words) for _ in range(n_words)).encode()
        for unit in ("byte", "char"):
            exp_ids, exp_spans = NM.encode_spans_normalized(text, VOCAB, flags, unit)
            ids, offs = gv.encode_with_offsets(text, unit=unit)
            assert np.array_equal(ids, np.array(exp_ids, dtype=np.int32))
            assert np.array_equal(offs, np.array(exp_spans, dtype=np.uint32).reshape(-1, 2))

    gv.set_option(W.WP_OPT_NORMALIZE, flags)
    try:
        n_large = 80000  # two code points or more per word: 8 bytes per code point in norm_map
        assert n_large * 2 * 8 > GROW
        small_then_large(gv, run, 64, n_large, 8)
    finally:
        gv.set_option(W.WP_OPT_NORMALIZE, 0)


# ---- the grouping layers ----------------------------------------------------------------------------------------------


def _words_text(n_words, seed):
    """n_words words of 1 to 4 letters"""
    rng = random.Random(seed)
    return " ".join("".join(rng.choice(LETTERS) for _ in range(rng.randint(1, 4))) for _ in range(n_words)).encode()


@pytest.mark.gpu
def test_count_words(gv):
    def run(text):
        exp = known.get(id(text)) or CM.count_words(text, order="count")
        got = gv.count_words(text, order="count", index=True, raw=True)
        assert got["words"].tobytes() == exp["pool"]
        for k in ("word_off", "counts", "word_index"):
            assert got[k].tolist() == exp[k], k
        st = gv.count_stats()
        assert {k: st[k] for k in exp["stats"]} == exp["stats"]

    n_large = 325000
    large = _words_text(n_large, 91)
    exp = CM.count_words(large, order="count")  # (the model takes 2.9 s at this size)
    known = {id(large): exp}
    # the text in text_buf and its valid UTF-8 in norm_buf; 17 words of 32 bits and 2 of 64 per word in count_words; the
    # pool, an offset and a count per kept word and the index in count_out.  count_aux holds three words per 2048 bytes
    # of text: no text a test can afford makes it grow.
    assert len(large) + 64 > GROW and (17 * 4 + 2 * 8) * n_large > GROW
    assert len(exp["pool"]) + 16 * len(exp["counts"]) + 4 * n_large > GROW
    small_then_large(gv, run, _words_text(64, 90), large, _words_text(8, 89))


def _table(n_words, alphabet, max_len, seed):
    """n_words distinct words in random order, with counts: (words as bytes, counts, pool, word_off)"""
    rng = random.Random(seed)
    words = set()
    while len(words) < n_words:
        words.add("".join(rng.choice(alphabet) for _ in range(rng.randint(1, max_len))))
    words = sorted(words)
    rng.shuffle(words)
    words = [w.encode() for w in words]
    off = np.zeros(n_words + 1, dtype=np.int64)
    np.cumsum([len(w) for w in words], out=off[1:])
    return words, [rng.randint(1, 40) for _ in words], np.frombuffer(b"".join(words), dtype=np.uint8), off


@pytest.mark.gpu
def test_learn_vocab(gv):
    kw = dict(lower_thresh=2, upper_thresh=2, num_iterations=2, max_token_chars=8, max_unique_chars=0, slack=1 << 20)

    def run(case):
        words, counts, pool, off = case
        exp = known.get(id(case)) or LM.learn(words, counts, 1 << 20, reserved=[b"[PAD]", b"[UNK]"], **kw)
        got = gv.learn_vocab({"words": pool, "word_off": off, "counts": counts, "terminator": None}, 1 << 20, reserved=("[PAD]", "[UNK]"), **kw)
        assert got["tokens"] == exp["tokens"] and got["scores"].tolist() == exp["scores"] and got["thresh"] == exp["thresh"] == 2
        st = gv.learn_stats()
        assert {k: st[k] for k in exp["stats"]} == exp["stats"]

    large = _table(60000, LETTERS[:16], 5, 92)  # (the model takes 1.8 s on this table)
    n, n_bytes = len(large[0]), large[2].size
    exp = LM.learn(large[0], large[1], 1 << 20, reserved=[b"[PAD]", b"[UNK]"], **kw)
    known = {id(large): exp}
    n_listed = len(exp["tokens"]) - 2 - 2 * exp["stats"]["n_chars"]
    # the pool, the offsets and the counts in learn_in; 66 bytes per occurrence in learn_items; 32 per token in
    # learn_groups; room for the longest possible text of every listed token in learn_out
    assert n_bytes + 16 * n > GROW and 66 * exp["stats"]["n_occurrences"] > GROW and 32 * exp["stats"]["n_tokens"] > GROW
    assert (4 * 64 + 3) * n_listed > GROW
    # learn_aux holds two tables of 0x110000 words from the small call on; 36 bytes per byte of the pool come on top
    assert 36 * n_bytes > GROW + 2 * 4 * 0x110000 // 16
    small_then_large(gv, run, _table(31, "ab", 6, 93), large, _table(8, "abc", 3, 94))


def _ragged_rows(n_rows, seed):
    """n_rows text rows of 0 to 9 bytes drawn from a pool of 200: (data uint8, row_off)"""
    rng = random.Random(seed)
    pool = [bytes(rng.randrange(97, 101) for _ in range(rng.randint(0, 9))) for _ in range(200)]
    rows = [rng.choice(pool) for _ in range(n_rows)]
    off = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    return np.frombuffer(b"".join(rows), dtype=np.uint8), off


def _table_equal(got, exp, keys, want, dtype):
    """the arrays of a dedup or neardup result against the model's; the keys of the two forms of the output arena"""
    assert sorted(got) == sorted(keys + (("inverse", "data", "row_off") if want else ()))
    for k in got:
        if k == "data":
            assert got[k].dtype == dtype and got[k].tobytes() == exp[k]
        elif k != "signatures":
            assert got[k].tolist() == exp[k], k


N_RAGGED = 280000  # rows of the large batch of dedup and neardup: 4 bytes of `inverse` per row are all that grows their output arenas


@pytest.mark.gpu
def test_dedup_rows(gv):
    def run(case):
        data, off = case
        exp = DDM.dedup_rows(data.tobytes(), off, data.dtype.itemsize)
        for want in (True, False):  # (the two layouts of dedup_out alternate)
            got = gv.dedup_rows(data, off, inverse=want, compact=want, raw=True)
            _table_equal(got, exp, ("first", "kept", "counts"), want, data.dtype)
            st = gv.dedup_stats()
            assert {k: st[k] for k in exp["stats"]} == exp["stats"]

    large = _ragged_rows(N_RAGGED, 95)
    # the offsets in dedup_in; 23 words per row in dedup_rows; the inverse alone in dedup_out (the model takes 0.25 s)
    assert 8 * (N_RAGGED + 1) > GROW and 23 * 4 * N_RAGGED > GROW and 4 * N_RAGGED > GROW
    small_then_large(gv, run, _cells(31, 0, 96), large, _cells(8, 4, 97))


@pytest.mark.gpu
def test_neardup_rows(gv):
    spec = dict(shingle=2, n_perm=4, bands=2)

    def run(case):
        data, off = case
        exp = known.get(id(case)) or NDM.neardup_rows(data.tobytes(), off, data.dtype.itemsize, **spec)
        for want in (True, False):  # (the two layouts of neardup_out alternate)
            got = gv.neardup_rows(data, off, inverse=want, compact=want, signatures=want, raw=True, **spec)
            _table_equal(got, exp, ("cluster", "kept", "counts") + (("signatures",) if want else ()), want, data.dtype)
            if want:
                assert np.array_equal(got["signatures"], exp["signatures"])
            st = gv.neardup_stats()
            assert {k: st[k] for k in exp["stats"]} == exp["stats"]

    large = _ragged_rows(N_RAGGED, 95)
    known = {id(large): NDM.neardup_rows(large[0].tobytes(), large[1], 1, **spec)}  # (the model takes 1.1 s)
    n_live = N_RAGGED - known[id(large)]["stats"]["n_empty"]
    # the offsets in neardup_in; 12 words and 4 signature slots per row in neardup_rows; 60 bytes per band of a row with
    # elements in neardup_items; the inverse alone in neardup_out
    assert 8 * (N_RAGGED + 1) > GROW and (12 + 4) * 4 * N_RAGGED > GROW and 60 * 2 * n_live > GROW and 4 * N_RAGGED > GROW
    small_then_large(gv, run, _cells(31, 0, 98), large, _cells(8, 4, 99))


# ---- the window layers (window_path.h) ----------------------------------------------------------------------------------


def _window_equal(got, exp, keys):
    """the arrays of an overlap or repeat result against the model's; `keys`: what the call was asked for"""
    assert sorted(got) == sorted(keys)
    for k in got:
        if k in ("data", "cut_data"):
            assert (got[k] if isinstance(got[k], bytes) else got[k].tobytes()) == exp[k], k
        else:
            assert got[k].tolist() == exp[k], k


@pytest.mark.gpu
def test_overlap_rows(gv):
    base = ("hits", "first_hit", "first_ref", "covered")

    def run(case):
        (data, off), (rdata, roff) = case
        exp = known.get(id(case)) or OM.overlap_rows(data.tobytes(), off, rdata.tobytes(), roff, data.dtype.itemsize, ngram=3)
        for want in (True, False):  # (the two layouts of overlap_items, overlap_rows and overlap_out alternate)
            got = gv.overlap_rows(data, off, rdata, roff, ngram=3, mask=want, ref=want, compact=want, raw=True)
            _window_equal(got, exp, base + (("mask", "ref_hits", "kept", "data", "row_off") if want else ()))
            st = gv.overlap_stats()
            assert {k: st[k] for k in exp["stats"]} == exp["stats"]

    large = (_ragged_rows(N_RAGGED, 95), _ragged_rows(N_RAGGED, 100))
    exp = OM.overlap_rows(large[0][0].tobytes(), large[0][1], large[1][0].tobytes(), large[1][1], 1, ngram=3)
    known = {id(large): exp}
    n_elems, n_ref_elems, n_kept = large[0][0].size, large[1][0].size, len(exp["kept"])
    assert 0 < n_kept < N_RAGGED and exp["stats"]["n_ref_distinct"] == 64  # (long runs; the kept rows are a real subset)
    # the data and the offsets in overlap_in and in overlap_ref_in; 13 words per corpus row in overlap_rows; 7 words per
    # corpus element in overlap_items; the kept rows, their offsets and the room of the input in overlap_out
    assert n_elems + 8 * (N_RAGGED + 1) > GROW and n_ref_elems + 8 * (N_RAGGED + 1) > GROW and 13 * 4 * N_RAGGED > GROW
    assert 7 * 4 * n_elems > GROW and 12 * n_kept + n_elems > GROW
    small31, small8 = _cells(31, 0, 101), _cells(8, 4, 102)
    small_then_large(gv, run, (small31, small31), large, (small8, small8))


@pytest.mark.gpu
def test_repeat_rows(gv):
    base = ("repeats", "first_repeat", "first_src_row", "first_src_pos", "covered")

    def text(cells):  # (WP_REPEAT_UTF8 takes text)
        return (cells[0] % 4 + 97).astype(np.uint8), cells[1]

    def run(case):
        data, off = case
        exp = known.get(id(case)) or RM.repeat_rows(data.tobytes(), off, 1, ngram=3, scope=0, utf8=True)
        for want in (True, False):  # (the two layouts of repeat_items and repeat_out alternate; the wait of utf8 comes and goes)
            got = gv.repeat_rows(data, off, ngram=3, scope=0, mask=want, src=want, compact=want, cut=want, utf8=want)
            _window_equal(got, exp, base + (("mask", "src", "kept", "data", "row_off", "cut_data", "cut_off") if want else ()))
            st = gv.repeat_stats()
            assert {k: st[k] for k in exp["stats"]} == dict(exp["stats"], n_cut_elems=exp["stats"]["n_cut_elems"] if want else 0)

    large = _ragged_rows(N_RAGGED, 95)  # (ASCII: every window lies between code point boundaries, with the flag and without)
    exp = RM.repeat_rows(large[0].tobytes(), large[1], 1, ngram=3, scope=0, utf8=True)
    known = {id(large): exp}
    n_elems, n_kept = large[0].size, len(exp["kept"])
    assert 0 < n_kept < N_RAGGED and exp["stats"]["n_distinct"] == 64
    # the data and the offsets in repeat_in; 14 words per row in repeat_rows; 5 words per element in repeat_items; the
    # kept rows and the cut, each with its offsets and the room of the input, in repeat_out
    assert n_elems + 8 * (N_RAGGED + 1) > GROW and 14 * 4 * N_RAGGED > GROW and 5 * 4 * n_elems > GROW
    assert 12 * n_kept + 8 * (N_RAGGED + 1) + 2 * n_elems > GROW
    small_then_large(gv, run, text(_cells(31, 0, 103)), large, text(_cells(8, 4, 104)))
