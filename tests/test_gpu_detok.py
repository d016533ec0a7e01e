"""wp_detokenize / wp_detokenize_device on the GPU against the Python model (tests/detok_model.py): text, text_off and
statistics byte for byte.  The shapes sit at the kernels' edges (csrc/detok.h): T = kDetokTile slots per tile, W =
kDetokTripWords words per write trip — tile and row boundaries, carries across tiles, empty rows, the four byte
alignments of a row's and a tile's text, pieces from one byte to more than a write trip — not at workload size; one
case at 2^22 + 3 cells is checked against the numpy form of the model."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import detok_model as M
import wordpiece_amd as W

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")
T = 2048  # kDetokTile
WORDS = 256  # kDetokTripWords
LONG = "q" * (4 * WORDS + 477)  # one piece longer than a write trip of 4 * W bytes
WIDTHS = (1, 2, 3, 4, 5, 63, 64, 65)
VOCAB = (["[UNK]", "[CLS]", "[SEP]", "[PAD]", "[MASK]", "a", "##a", "é", "##é", "中", "##中", "\U0001f600",
          "##\U0001f600", ".", "##.", ",", "?", "!", "'", "n't", "##n't", "'m", "'s", "'ve", "'re", "do not", "##do not",
          "do", "not", "x y", "###", "#", "!!", "café", "is n't", LONG, "##" + LONG] +
         ["b" * k for k in WIDTHS[1:]] + ["##" + "c" * k for k in WIDTHS[1:]])
V = len(VOCAB)
ID = {t: i for i, t in enumerate(VOCAB)}
MALFORMED = ID["!!"]
A, CA, PAD, SEP = ID["a"], ID["##a"], ID["[PAD]"], ID["[SEP]"]  # "a": 1 byte as form0, 2 as form1; "##a": 3 and 1
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
OUTSIDE = [-1, V, I32_MIN, I32_MAX, MALFORMED]


def cont(k):
    """the continuation token whose form1 has k bytes (and whose form0 has k + 2)"""
    return CA if k == 1 else ID["##" + "c" * k]


def word(k):
    """the word-initial token whose form0 has k bytes (and whose form1 has k + 1)"""
    return A if k == 1 else ID["b" * k]


@pytest.fixture(scope="module")
def gv():
    return W.Vocab(VOCAB)


@pytest.fixture(scope="module")
def model(gv):
    m = M.Model.from_vocab(gv)
    assert m.lines == [t.encode("utf-8") for t in VOCAB] and m.malformed == {MALFORMED}
    return m


def check(gv, model, ids, row_splits=None, lengths=None, skip_ids=(), clean=True, terminator=None):
    text, off = gv.detokenize(ids, row_splits=row_splits, lengths=lengths, skip_ids=skip_ids, cleanup=clean,
                              terminator=terminator, raw=True)
    exp_text, exp_off, exp_stats = model.detokenize(ids, row_splits=row_splits, lengths=lengths, skip_ids=skip_ids,
                                                    clean=clean, terminator=terminator)
    assert off.tolist() == exp_off
    if text != exp_text:
        at = next(i for i in range(min(len(text), len(exp_text))) if text[i] != exp_text[i]) if len(text) == len(exp_text) else -1
        raise AssertionError("text differs at byte %d of %d / %d: %r != %r" % (at, len(text), len(exp_text),
                                                                                text[max(at - 8, 0):at + 8],
                                                                                exp_text[max(at - 8, 0):at + 8]))
    assert gv.detok_stats() == exp_stats
    return text, exp_off


def mixed_ids(rng, n):
    """mostly short tokens, some skipped ([PAD], [SEP]) and some dropped"""
    pool = [A, CA, ID["é"], ID["##中"], ID["."], ID["n't"], ID["do not"], cont(5), word(4), ID["###"]]
    return [rng.choice(OUTSIDE) if rng.random() < 0.04 else rng.choice([PAD, SEP]) if rng.random() < 0.08 else rng.choice(pool)
            for _ in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [T - 1, T, T + 1, 3 * T + 2])
def test_cell_counts_as_one_row(gv, model, n):
    ids = mixed_ids(random.Random(n), n)
    for term in (None, "\n"):
        check(gv, model, ids, row_splits=[0, n], skip_ids=[PAD, SEP], terminator=term)


@pytest.mark.gpu
def test_row_boundaries(gv, model):
    rng = random.Random(3)
    ids = mixed_ids(rng, T + 1)
    check(gv, model, ids, row_splits=list(range(T + 2)), skip_ids=[PAD], terminator="\n")  # T + 1 rows of one cell
    check(gv, model, ids, row_splits=list(range(T + 2)), skip_ids=[PAD])
    ids = mixed_ids(rng, 2 * T + 7)
    for edge in (T - 1, T, T + 1):  # a boundary on a tile edge and one cell to either side, alone and all three
        check(gv, model, ids, row_splits=[0, edge, len(ids)], terminator="\n")
        check(gv, model, ids, row_splits=[0, 5, edge, 2 * T, len(ids)])
    check(gv, model, ids, row_splits=[0, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, len(ids)], terminator=0)


@pytest.mark.gpu
@pytest.mark.parametrize("gap", [2 * T + 3, 2 * T, 3 * T, T - 1, 2 * T - 5])
def test_carry_across_tiles(gv, model, gap):
    """A row whose first `gap` cells are all skipped or dropped: the next cell is the row's first kept one (form0),
    although its row began tiles ago — with gap 2T and 3T it is the first cell of its tile."""
    rng = random.Random(gap)
    dead = [rng.choice([PAD, SEP, -1, V, MALFORMED]) for _ in range(gap)]
    tail = [word(3), CA, A, PAD, word(2)]
    for front in ([], [A, CA], [PAD] * 3, [A] * (T - 2)):  # the row in front ends with / without a kept cell
        ids = front + dead + tail
        text, off = check(gv, model, ids, row_splits=[0, len(front), len(ids)], skip_ids=[PAD, SEP], terminator="\n")
        assert text[off[1]:off[2]] == b"bbba a bb\n"
    # the same stretch inside a row that has a kept cell in front of it: form1 after the gap
    ids = [A] + dead + tail
    text, off = check(gv, model, ids, row_splits=[0, len(ids)], skip_ids=[PAD, SEP])
    assert text == b"a bbba a bb"
    # the carry ends at a row start inside a stretch of dead tiles: an empty row in between
    ids = [A] + dead + tail
    cut = min(T + 5, gap)
    text, off = check(gv, model, ids, row_splits=[0, cut, cut, len(ids)], skip_ids=[PAD, SEP], terminator="\n")
    assert text == b"a\n\nbbba a bb\n"


@pytest.mark.gpu
def test_empty_rows(gv, model):
    ids = [A, CA, word(3), A, A]
    patterns = [[0, 0, 5], [0, 5, 5], [0, 2, 2, 5], [0, 0, 0, 0, 2, 2, 2, 5, 5, 5], [0, 0], [0, 0, 0, 0, 0]]
    for splits in patterns:
        for term in (None, "\n", 255):
            check(gv, model, ids[:splits[-1]], row_splits=splits, terminator=term)
    # more empty rows than a tile has slots, around a tile edge, and nothing but empty rows
    ids = mixed_ids(random.Random(5), T + 3)
    splits = [0] * 300 + [T] * (T + 9) + [T + 3] * 70
    for term in (None, "\n"):
        check(gv, model, ids, row_splits=splits, terminator=term)
        check(gv, model, [], row_splits=[0] * (T + 2), terminator=term)


@pytest.mark.gpu
def test_alignment_of_rows_tiles_and_totals(gv, model):
    # a total of 1..5 bytes: one kept cell
    for k in (1, 2, 3, 4, 5):
        text, _ = check(gv, model, [PAD, word(k)], row_splits=[0, 2], skip_ids=[PAD])
        assert len(text) == k
        check(gv, model, [word(k)], row_splits=[0, 0, 1], terminator="\n")
    # rows whose text starts at each alignment: rows of 1, 2, 3, 4 and 5 bytes in every order of a few
    rng = random.Random(9)
    for trial in range(6):
        ks = [rng.choice((1, 2, 3, 4, 5)) for _ in range(37)]
        ids = [word(k) for k in ks]
        for term in (None, "\n"):
            check(gv, model, ids, row_splits=list(range(len(ids) + 1)), terminator=term)
    # a tile's byte range starting and ending at each alignment: tile 0 holds T one-byte pieces but for its first cell
    # (form0, 3 bytes) and one piece of k bytes; tile 1 the same with a piece of j bytes
    for k in (1, 2, 3, 4):
        for j in (1, 2, 3, 4):
            ids = [CA] * (2 * T + 1)
            ids[7], ids[T + 9] = cont(k), cont(j)
            text, _ = check(gv, model, ids, row_splits=[0, len(ids)])
            assert len(text) == 2 * T + 1 + 2 + (k - 1) + (j - 1)


@pytest.mark.gpu
def test_piece_lengths(gv, model):
    for k in WIDTHS:
        ids = [word(k), cont(k), word(k), PAD, cont(k)]
        text, _ = check(gv, model, ids, row_splits=[0, 5], skip_ids=[PAD], clean=False)
        assert len(text) == k + k + (k + 1) + k
        check(gv, model, ids * 3, row_splits=[0, 4, 9, 15], terminator="\n")
    long_w, long_c = ID[LONG], ID["##" + LONG]
    assert len(LONG) > 4 * WORDS
    text, _ = check(gv, model, [A, long_c, long_w, CA], row_splits=[0, 4])  # a piece spans write trips
    assert len(text) == 1 + len(LONG) + 1 + len(LONG) + 1
    for shift in (0, 1, 2, 3):  # the long piece as the last cell of a tile and the first of the next
        ids = [CA] * (T - 1 - shift) + [A] * shift + [long_c, long_w, long_c] + [CA] * 3
        check(gv, model, ids, row_splits=[0, len(ids)])
        check(gv, model, ids, row_splits=[0, T - 1, T, len(ids)], terminator="\n")


@pytest.mark.gpu
@pytest.mark.parametrize("max_len", [1, 3, 64, 65, 200])
def test_padded_layout(gv, model, max_len):
    rng = random.Random(max_len)
    n_rows = {1: T + 3, 3: 700, 64: 33, 65: 33, 200: 11}[max_len]
    ids = np.array(mixed_ids(rng, n_rows * max_len), dtype=np.int64).reshape(n_rows, max_len)
    for term in (None, "\n"):
        check(gv, model, ids, skip_ids=[PAD, SEP], terminator=term)  # lengths == NULL: full rows
        lens = [rng.choice([0, max_len, max_len + 1, 10 ** 6, -1, -10 ** 6, rng.randrange(max_len + 1)]) for _ in range(n_rows)]
        check(gv, model, ids, lengths=lens, skip_ids=[PAD, SEP], terminator=term)
    # garbage behind the lengths shows neither in the text nor in the statistics
    lens = np.array([rng.randrange(max_len + 1) for _ in range(n_rows)])
    dirty = ids.copy()
    for r in range(n_rows):
        dirty[r, lens[r]:] = rng.choice([A, I32_MAX, -7, MALFORMED])
    a = gv.detokenize(dirty, lengths=lens, skip_ids=[PAD], terminator="\n", raw=True)
    sa = gv.detok_stats()
    b = gv.detokenize(ids, lengths=lens, skip_ids=[PAD], terminator="\n", raw=True)
    assert a[0] == b[0] and a[1].tolist() == b[1].tolist() and sa == gv.detok_stats() and sa["n_cells"] == int(lens.sum())
    check(gv, model, dirty, lengths=lens, skip_ids=[PAD], terminator="\n")
    check(gv, model, ids, lengths=[0] * n_rows, terminator="\n")


@pytest.mark.gpu
def test_ids_outside_and_skipped(gv, model):
    ids = [A] + OUTSIDE + [CA, PAD] + OUTSIDE + [word(2), SEP, A]
    text, _ = check(gv, model, ids, row_splits=[0, len(ids)])
    assert gv.detok_stats()["n_dropped"] == 10 and gv.detok_stats()["n_skipped"] == 0
    check(gv, model, OUTSIDE * 3, row_splits=[0, 4, 15], terminator="\n")  # rows of dropped cells only
    check(gv, model, ids, row_splits=[0, 3, len(ids)], skip_ids=[PAD])
    assert gv.detok_stats()["n_skipped"] == 1
    eight = [PAD, SEP, ID["[CLS]"], ID["[MASK]"], ID["[UNK]"], ID["."], ID["do not"], CA]
    text, _ = check(gv, model, ids + eight, row_splits=[0, 3, len(ids) + 8], skip_ids=eight, terminator="\n")
    assert gv.detok_stats()["n_skipped"] == 3 + 8
    # a skip id outside the vocabulary (or malformed) is dropped, not skipped
    check(gv, model, ids, row_splits=[0, len(ids)], skip_ids=[-1, V, I32_MAX, MALFORMED, PAD])
    assert gv.detok_stats()["n_dropped"] == 10 and gv.detok_stats()["n_skipped"] == 1


@pytest.mark.gpu
def test_cleanup_on_off_and_alternating():
    v = W.Vocab(VOCAB)  # a handle of its own: the table is built by its first call, whichever cleanup that has
    m = M.Model.from_vocab(v)
    rng = random.Random(21)
    pool = [ID[t] for t in (".", "##.", ",", "?", "!", "'", "n't", "##n't", "'m", "'s", "'ve", "'re", "do not", "##do not",
                            "do", "not", "x y", "is n't", "a", "##a", "café")]
    ids = [rng.choice(pool) for _ in range(T + 40)]
    splits = sorted(rng.randrange(len(ids) + 1) for _ in range(50))
    splits = [0] + splits + [len(ids)]
    texts = {}
    for clean in (False, True, False, True, True, False):
        texts[clean], _ = check(v, m, ids, row_splits=splits, clean=clean, terminator="\n")
    assert texts[True] != texts[False] and b" don't" in texts[True] and b" do not" in texts[False]


def _torch():
    import torch
    return torch


def _tensor_call(gv, ids, **kw):
    text, off = gv.detokenize_tensor(ids, **kw)
    return bytes(text.cpu().numpy().tobytes()), off.cpu().tolist()


@pytest.mark.gpu
def test_device_entry_point(gv, model):
    torch = _torch()
    rng = random.Random(31)
    ids = mixed_ids(rng, 2 * T + 100)
    splits = [0, 3, 3, T, T + 1, 2 * T + 100]
    # dirty bytes behind (and in front of) the ids: a view into a larger buffer of garbage
    big = torch.full((len(ids) + 4096,), A, dtype=torch.int32, device="cuda")
    big[8:8 + len(ids)] = torch.tensor(ids, dtype=torch.int64).to(torch.int32).cuda()
    d_ids = big[8:8 + len(ids)]
    d_splits = torch.tensor(splits, dtype=torch.int64, device="cuda")
    exp_text, exp_off, exp_stats = model.detokenize(ids, row_splits=splits, skip_ids=[PAD], terminator="\n")
    assert _tensor_call(gv, d_ids, row_splits=d_splits, skip_ids=[PAD], terminator="\n") == (exp_text, exp_off)
    assert gv.detok_stats() == exp_stats
    # a second call that reuses the buffers with a shorter result, as views of the library's memory
    short, s_splits = ids[:70], [0, 10, 70]
    e2 = model.detokenize(short, row_splits=s_splits, terminator="\n")
    text, off = gv.detokenize_tensor(d_ids[:70], row_splits=torch.tensor(s_splits, device="cuda"), terminator="\n", copy=False)
    assert text.dtype == torch.uint8 and off.dtype == torch.int64
    assert (bytes(text.cpu().numpy().tobytes()), off.cpu().tolist()) == (e2[0], e2[1]) and gv.detok_stats() == e2[2]
    # a bare 1-d tensor is one row; a 2-d tensor is a padded batch, with and without lengths
    e3 = model.detokenize(short)
    assert _tensor_call(gv, d_ids[:70].contiguous()) == (e3[0], e3[1])
    batch = torch.tensor(ids[:66 * 31], dtype=torch.int64).to(torch.int32).reshape(66, 31).cuda()
    lens = [rng.choice([0, 31, 40, -2, 7]) for _ in range(66)]
    e4 = model.detokenize(np.array(ids[:66 * 31]).reshape(66, 31), lengths=lens, skip_ids=[PAD, SEP], clean=False, terminator=0)
    assert _tensor_call(gv, batch, lengths=torch.tensor(lens, dtype=torch.int32, device="cuda"), skip_ids=[PAD, SEP],
                        cleanup=False, terminator=0) == (e4[0], e4[1])
    assert gv.detok_stats() == e4[2]
    e5 = model.detokenize(np.array(ids[:66 * 31]).reshape(66, 31))
    assert _tensor_call(gv, batch) == (e5[0], e5[1])
    # no rows, and rows without cells
    assert _tensor_call(gv, d_ids[:0], row_splits=torch.zeros(1, dtype=torch.int64, device="cuda")) == (b"", [0])
    assert _tensor_call(gv, d_ids[:0], row_splits=torch.zeros(4, dtype=torch.int64, device="cuda"), terminator="\n") == \
        (b"\n\n\n", [0, 1, 2, 3])
    # row_splits are checked in a kernel: WP_ERR_ARG before any text
    for bad in ([1, 3, 70], [0, 40, 30, 70], [0, -1, 70]):
        with pytest.raises(W.WordPieceError, match="row_splits"):
            gv.detokenize_tensor(d_ids[:70], row_splits=torch.tensor(bad, device="cuda"))
    assert _tensor_call(gv, d_ids[:70].contiguous()) == (e3[0], e3[1])  # the handle is fine afterwards


LETTERS = "abcdefghijklmnopqrstuvwxyz"
LETTER_VOCAB = ["[UNK]", "[CLS]", "[SEP]", "[PAD]"] + list(LETTERS) + ["##" + ch for ch in LETTERS] + ["the", "##ing", "##ed", "qu"]


def letter_docs(rng, n_docs):
    docs = []
    for _ in range(n_docs):
        words = ["".join(rng.choice(LETTERS) for _ in range(rng.choice([1, 2, 3, 7, 12]))) for _ in range(rng.choice([0, 1, 2, 5, 30]))]
        docs.append(" ".join(words))
    return docs


@pytest.mark.gpu
def test_round_trip_of_encode_rows():
    """Lower-case words over a letters vocabulary (no [UNK] possible), single blanks, none at either end:
    detokenize(encode_rows(docs), cleanup off, terminator newline) is the joined text and its doc_off."""
    torch = _torch()
    v = W.Vocab(LETTER_VOCAB)
    rng = random.Random(41)
    docs = letter_docs(rng, 400)
    joined, doc_off = W.join_docs(docs)
    ids, splits = v.encode_rows(docs=docs)[:2]
    assert v.unk_id not in set(ids.tolist()) and len(ids) > 2 * T
    text, off = v.detokenize(ids, row_splits=splits, cleanup=False, terminator="\n", raw=True)
    assert text == joined and off.tolist() == doc_off.tolist()
    assert v.detokenize(ids, row_splits=splits, cleanup=False) == docs
    # on the device: the tensors of encode_rows_tensor fed straight in (copies, and the library's own views)
    d_text = torch.frombuffer(bytearray(joined), dtype=torch.uint8).cuda()
    d_off = torch.tensor(doc_off, dtype=torch.int64, device="cuda")
    for copy in (True, False):
        d_ids, d_splits = v.encode_rows_tensor(d_text, d_off, copy=copy)
        t, o = v.detokenize_tensor(d_ids, row_splits=d_splits, cleanup=False, terminator="\n")
        assert torch.equal(t, d_text) and torch.equal(o, d_off)


@pytest.mark.gpu
def test_at_size(gv, model):
    rng = np.random.default_rng(51)
    n = 2 ** 22 + 3
    n_rows = 40000
    cuts = np.sort(rng.integers(0, n + 1, size=n_rows - 1 - 2000))
    cuts = np.sort(np.concatenate([cuts, rng.choice(cuts, size=2000)]))  # some rows of no cell
    splits = np.concatenate([[0], cuts, [n]]).astype(np.int64)
    ids = rng.integers(0, V, size=n).astype(np.int64)
    ids[np.isin(ids, [ID[LONG]] + [word(k) for k in (63, 64, 65)])] = A  # (short pieces: the model's index arrays stay small)
    ids[np.isin(ids, [ID["##" + LONG]] + [cont(k) for k in (63, 64, 65)])] = CA
    out = rng.random(n) < 0.01
    ids[out] = rng.choice(np.array(OUTSIDE), size=int(out.sum()))
    assert (np.diff(splits) == 0).sum() >= 2000
    exp_text, exp_off, exp_stats = model.detokenize_np(ids, splits, skip_ids=[PAD, SEP], clean=True, terminator="\n")
    text, off = gv.detokenize(ids.astype(np.int32), row_splits=splits, skip_ids=[PAD, SEP], terminator="\n", raw=True)
    assert np.array_equal(off, exp_off) and gv.detok_stats() == exp_stats
    assert len(text) == len(exp_text) and np.array_equal(np.frombuffer(text, dtype=np.uint8), exp_text)


def geometry_grid(gv, model):
    """a small run over both layouts for the bounds-checking build; returns the number of calls"""
    rng = random.Random(61)
    n = 0
    for cells in (T - 1, 2 * T + 3):
        ids = mixed_ids(rng, cells) + [ID[LONG]]
        for term in (None, "\n"):
            check(gv, model, ids, row_splits=[0, 0, 5, T - 3, len(ids)], skip_ids=[PAD], terminator=term)
            n += 1
    batch = np.array(mixed_ids(rng, 90 * 65), dtype=np.int64).reshape(90, 65)
    check(gv, model, batch, lengths=[rng.randrange(-3, 70) for _ in range(90)], terminator="\n")
    return n + 1


@pytest.mark.gpu
def test_bounds_checking_build(tmp_path):
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "detok_dbg_run.py"
    script.write_text('''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import wordpiece_amd as W
import detok_model as M
from test_gpu_detok import VOCAB, geometry_grid
gv = W.Vocab(VOCAB)
gv.encode("a a")
assert gv.stats()["reserved0"] == 1, "not the bounds-checking build"
assert geometry_grid(gv, M.Model.from_vocab(gv)) == 5
print("DETOK_DEBUG_OK")
''' % (os.path.dirname(PKG), HERE))
    env = dict(os.environ, WP_LIB=dbg)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "DETOK_DEBUG_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
