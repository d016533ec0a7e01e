"""GPU tests (-m gpu) of the special-tokens entry points (wp_linear_encode_special / _rows and their device forms; kernels:
csrc/special.h) against the Python model (tests/special_model.py), exactly, in bytes, code points and without a unit.
The shapes sit at the kernels' edges: 16 bytes per lane, 1 KB rows of the code-point count, 16 KB tiles of the match,
2048 output cells per workgroup of the merge."""
import os
import subprocess
import sys

import numpy as np
import pytest

import normalize_model as NM
import rows_model as R
import special_model as S
import wordpiece_amd as W

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")
UNITS = (None, "byte", "char")
LONG = "[" + "q" * 62 + "]"  # a line of exactly 64 bytes
VOCAB = ["[UNK]", "[CLS]", "[SEP]", "[PAD]", "[MASK]", "[MASK2]", "[a]", LONG, "a", "##a", "b", "##b", "ab", "mask", "cafe", "hello",
         "##s", "é", "中", "[", "]", ".", "q", "##q", "MASK", "2", "##2"]
LISTED = ["[CLS]", "[SEP]", "[MASK]", "[MASK2]", "[a]", LONG]


@pytest.fixture(scope="module")
def gv():
    return W.Vocab(VOCAB)


@pytest.fixture(scope="module")
def model():
    return R.Model(VOCAB)


@pytest.fixture(scope="module")
def tab():
    return S.table(VOCAB, S.special_ids(VOCAB, LISTED))


def _b(x):
    return x if isinstance(x, (bytes, bytearray)) else x.encode("utf8")


def _dev(text):
    import torch
    return torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")


def _np(t):
    import torch
    return t.view(torch.int32).cpu().numpy().view(np.uint32) if t.dtype == torch.uint32 else t.cpu().numpy()


def _same_flat(got, unit, exp, label):
    ids, offs = (got, None) if unit is None else got
    assert ids.dtype == np.int32 and ids.tolist() == exp[0], label
    if unit is not None:
        assert offs.dtype == np.uint32 and offs.shape == (len(exp[0]), 2) and [tuple(o) for o in offs.tolist()] == exp[1], label


def flat_check(gv, enc, tab, text, label, tensor=True):
    """the host and the device entry point against the model in every unit; the statistics of the call"""
    text = _b(text)
    listed = sorted(tab.values())
    lits = S.find(text, tab)
    for unit in UNITS:
        exp = S.encode_special(enc, text, tab, unit)
        _same_flat(gv.encode_special(text, special_ids=listed, offsets=unit), unit, exp, (label, unit, "host"))
        if text:
            assert gv.special_stats() == dict(n_literals=len(lits), n_ids=len(exp[0]), n_rows=-1, n_listed=len(listed)), (label, unit)
            assert gv.stats()["offsets_unit"] == {None: -1, "byte": 0, "char": 1}[unit] and gv.stats()["n_ids"] == len(exp[0])
        if tensor and text:
            got = gv.encode_special_tensor(_dev(text), special_ids=listed, offsets=unit)
            _same_flat(_np(got) if unit is None else tuple(_np(t) for t in got), unit, exp, (label, unit, "device"))
    return len(lits)


def rows_check(gv, enc, tab, docs, label, route=1, tensor=True, only=None, units=UNITS):
    """explicit rows and the lines of the joined text (with and without the last newline) against the model per document
    (only: one of the three modes, units: some of the units, where the text is long)"""
    import torch
    text, starts = R.join_docs(docs)
    listed = sorted(tab.values())
    modes = [("explicit", text, starts, docs), ("lines", text, None, R.split_lines(text))]
    if text:
        modes.append(("lines, open end", text[:-1], None, R.split_lines(text[:-1])))
    for mode, t, off, rows in modes:
        if only is not None and mode != only:
            continue
        for unit in units:
            exp = S.encode_special_rows(enc, rows, tab, unit)
            got = gv.encode_special_rows(text=t, doc_offsets=off, special_ids=listed, offsets=unit)
            forms = [("host", got)]
            if tensor and t:
                d_off = None if off is None else torch.as_tensor(np.asarray(off, np.int64)).to("cuda:0")
                forms.append(("device", tuple(_np(x) for x in gv.encode_special_rows_tensor(_dev(t), d_off, special_ids=listed, offsets=unit))))
            for form, g in forms:
                where = (label, mode, unit, form)
                assert g[0].tolist() == exp[0] and g[1].dtype == np.int64 and g[1].tolist() == exp[1], where
                if unit is not None:
                    assert g[2].shape == (len(exp[0]), 2) and [tuple(o) for o in g[2].tolist()] == exp[2], where
            if t and not (off is not None and len(t) == len(rows)):  # (a call that reached the device)
                n_lits = sum(len(S.find(_b(d), tab)) for d in rows)
                assert gv.special_stats() == dict(n_literals=n_lits, n_ids=len(exp[0]), n_rows=len(rows), n_listed=len(listed)), (label, mode)
                assert gv.stats()["rows_route"] == route and gv.stats()["n_rows"] == len(rows), (label, mode)


EDGE_TEXTS = [
    "[MASK] a", "a [MASK]", "[MASK]", "a[MASK]b", "[CLS] hello [SEP]", "[MASK][MASK2][a]", "[a][a][a]", "[[MASK]]", "[mask]", "[MASK2",
    "ab [MASK2", "[MASK 2]", "[MASK2]2", "a" + LONG + "b", LONG, LONG + LONG, "[" + "q" * 63 + "]", "a[" + "q" * 63 + "] [a]",
    "[" + "q" * 61 + "]", "[" * 40, "[" * 33 + "a]", "]" * 20 + "[a]" + "[" * 20, "[a[a]]", "[a\n]", "[a] \n [a]", " [a] ", "\n[a]\n",
    "é[MASK]中[SEP]é", "中中[a]中", b"\xff[a]\xc3[MASK]\xe4\xb8[SEP]\x80", b"[a]\xc3", b"\xf0\x9f\x98[a]\xf0\x9f\x98\x80[a]", b"a\xc3[a", b"[MAS\xc3\xa9K] [a]",
    "cafe[MASK]s", "hellos[SEP]hellos", "x[MASK]x", "x [MASK] x", "Paris is the [MASK] of France.",
]


@pytest.mark.gpu
def test_edges_in_short_texts(gv, model, tab):
    n = sum(flat_check(gv, model, tab, t, t) for t in EDGE_TEXTS)
    assert n >= 40
    # a text of nothing but '[', over several tiles; and one where every '[' opens a candidate of 64 bytes that fails
    assert flat_check(gv, model, tab, "[" * 40000, "brackets") == 0
    assert flat_check(gv, model, tab, ("[" + "q" * 63) * 700 + LONG, "long candidates") == 1


@pytest.mark.gpu
def test_literal_at_the_end_of_the_text_and_cut_by_it(gv, model, tab):
    """The device entry point on a prefix of a longer buffer: the bytes behind nbytes are padding, whatever they hold.  A
    literal that ends exactly at nbytes counts; one that nbytes cuts does not, although the padding would complete it."""
    full = b"abc [MASK] ab [MASK] ab [a] abcd [MASK2] a"
    d_full = _dev(full + b"\0" * 64)
    listed = sorted(tab.values())
    assert full[14:20] == b"[MASK]" and full[24:27] == b"[a]" and full[33:40] == b"[MASK2]"
    for n, n_lits in ((20, 2), (16, 1), (28, 3), (24, 2), (36, 3), (40, 4), (4, 0), (8, 0), (12, 1)):
        text = full[:n]
        assert len(S.find(text, tab)) == n_lits
        for unit in UNITS:
            exp = S.encode_special(model, text, tab, unit)
            got = gv.encode_special_tensor(d_full[:n], special_ids=listed, offsets=unit)
            _same_flat(_np(got) if unit is None else tuple(_np(t) for t in got), unit, exp, (n, unit))
            assert gv.special_stats()["n_literals"] == n_lits
            rows = S.encode_special_rows(model, R.split_lines(text), tab, unit)
            g = gv.encode_special_rows_tensor(d_full[:n], None, special_ids=listed, offsets=unit)
            assert _np(g[0]).tolist() == rows[0] and _np(g[1]).tolist() == rows[1], (n, unit)


def _edge_text():
    """"[MASK2]" (7 bytes) starting at every distance 0..7 in front of a 16-byte, a 1 KB and a 16 KB boundary, in a
    filler of words, two-byte characters and line ends that the literals overwrite wherever they fall (so some stand
    beside the halves of a cut character)"""
    lit = b"[MASK2]"
    places = [16 * 5 * (d + 1) - d for d in range(8)] + [1024 * (d + 1) - d for d in range(8)] + [16384 * (d + 1) - d for d in range(8)]
    unit = "a é ab\nbé ".encode()
    buf = bytearray((unit * (9 * 16384 // len(unit) + 1))[:8 * 16384 + 100])
    for p in places:
        buf[p:p + len(lit)] = lit
    return bytes(buf), places


@pytest.mark.gpu
def test_literal_start_at_every_distance_from_a_lane_row_and_tile_edge(gv, model, tab):
    text, places = _edge_text()
    found = [p for p, _, _ in S.find(text, tab)]
    assert found == sorted(places) and len(found) == 24
    assert flat_check(gv, model, tab, text, "edges") == 24
    rows_check(gv, model, tab, R.split_lines(text), "edges by lines", only="lines, open end", units=("char",))
    rows_check(gv, model, tab, R.split_lines(text), "edges, explicit rows", only="explicit", units=("byte",))


@pytest.mark.gpu
def test_normalize_applies_to_the_blanked_text_only():
    vocab = ["[UNK]", "[MASK]", "[SEP]", "[mask]", "hello", "cafe", "##s", "world", "a"]

    class Uncased:
        @staticmethod
        def encode_with_offsets(text, unit):
            ids, spans = NM.encode_spans_normalized(text, vocab, 7, unit)
            return list(ids), [tuple(s) for s in spans]

    nv = W.Vocab(vocab, normalize=W.WP_NORM_BERT_UNCASED)
    tab = S.table(vocab, [1, 2])
    texts = ["Hello [MASK] CAF\u00c9S", "[MASK]HELLO[SEP]Caf\u00e9s[MASK]", "H\u00c9LLO [mask] [Mask] [MASK]",
             "\u00c0 [SEP]\u0301 A\u0300[MASK]\u00e1", "CAF\u00c9[MASK]\u200bWORLD [SEP]", "[MASK]", "\u0301[MASK]\u0301"]
    for t in texts:
        flat_check(nv, Uncased, tab, t, t)
    assert nv.encode_special("Hello [MASK] CAF\u00c9S", special_ids=[1, 2]).tolist() == [4, 1, 5, 6]
    rows_check(nv, Uncased, tab, texts + ["", "\u0301"], "uncased rows")
    # the lower-case line is ordinary text to the list, and a literal of its own where it is listed
    tab2 = S.table(vocab, [1, 3])
    flat_check(nv, Uncased, tab2, "[MASK] [mask] [Mask]", "both cases listed")


ROW_DOCS = ["[MASK] a b", "a b [SEP]", "[MASK]", "", "ab", "", "[SEP][MASK]", "a[a]b", "é[MASK2]中", "[", "mask [MASK", "MASK] [a]", LONG, "", "[CLS]"]


@pytest.mark.gpu
def test_rows_explicit_and_lines_on_both_routes(gv, model, tab):
    rows_check(gv, model, tab, ROW_DOCS, "joined route")
    rows_check(gv, model, tab, ["[MASK]"], "one row, one literal")
    rows_check(gv, model, tab, ["", "", ""], "empty rows")
    rows_check(gv, model, tab, ["[MASK]"] * 300 + [""] * 5 + ["a [SEP] a"] * 300, "many rows")
    # duplicate eligible lines: one encode per document
    vocab = VOCAB + ["ab", "a"]
    dv, dm = W.Vocab(vocab), R.Model(vocab)
    rows_check(dv, dm, S.table(vocab, S.special_ids(vocab, LISTED)), ROW_DOCS, "per-document route", route=0)
    # a listed line that repeats in the vocabulary: either copy may be listed, not both
    vocab = VOCAB + ["[MASK]"]
    rv, rm = W.Vocab(vocab), R.Model(vocab)
    for ids in ([4], [len(vocab) - 1]):
        rows_check(rv, rm, S.table(vocab, ids), ROW_DOCS[:7], "either copy %r" % ids, tensor=False)
    with pytest.raises(W.WordPieceError, match="id %d " % (len(vocab) - 1)):
        rv.encode_special("a", special_ids=[4, len(vocab) - 1])


@pytest.mark.gpu
def test_without_literals_and_with_an_empty_list_the_plain_call(gv, model, tab):
    listed = sorted(tab.values())
    for text in ("a b ab [ mask ] [MASK", "Paris is the [MASK] of France.\nab [SEP]\n\n[a]"):
        for ids in ([], listed):
            if ids and S.find(_b(text), tab):
                continue
            for unit in ("byte", "char"):
                a = gv.encode_special(text, special_ids=ids, offsets=unit)
                assert gv.special_stats() == dict(n_literals=0, n_ids=len(a[0]), n_rows=-1, n_listed=len(ids))
                b = gv.encode_with_offsets(text, unit=unit)  # (an encode: the special-tokens statistics start over)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                assert gv.special_stats()["n_literals"] == -1
                ra = gv.encode_special_rows(text=text, special_ids=ids, offsets=unit)
                rb = gv.encode_rows(text=text, offsets=unit)
                assert all(np.array_equal(x, y) for x, y in zip(ra, rb)) and len(ra) == 3
            assert np.array_equal(gv.encode_special(text, special_ids=ids), gv.encode(text))
            assert all(np.array_equal(x, y) for x, y in zip(gv.encode_special_rows(text=text, special_ids=ids), gv.encode_rows(text=text)))
    # None lists every line that may be listed
    assert gv.encode_special("[PAD][UNK] a").tolist() == [3, 0, 8]


def _periodic(model, tab, piece, reps, unit):
    """the model's result for piece * reps, from the piece alone: a piece that ends in a blank is encoded on its own"""
    ids, offs = S.encode_special(model, piece, tab, unit)
    step = len(piece) if unit == "byte" else len(piece.decode())
    all_ids = np.tile(np.asarray(ids, np.int32), reps)
    all_offs = (np.tile(np.asarray(offs, np.int64), (reps, 1)).reshape(reps, len(ids), 2) + (np.arange(reps) * step)[:, None, None]).reshape(-1, 2)
    return all_ids, all_offs.astype(np.uint32)


@pytest.mark.gpu
def test_two_hundred_thousand_literals_in_two_megabytes(gv, model, tab):
    """every scan crosses tiles: about 2 * 10^5 literals in 2 MB, with a period of 21 bytes against the 16-byte lanes"""
    piece = "é [MASK]ab [SEP] ab\n".encode()
    assert len(piece) == 21 and piece.endswith(b"\n")
    reps = 100_000
    for unit in ("byte", "char"):  # the periodic statement is the model's, checked at a size the model runs at
        three = S.encode_special(model, piece * 3, tab, unit)
        p_ids, p_offs = _periodic(model, tab, piece, 3, unit)
        assert three[0] == p_ids.tolist() and [tuple(o) for o in p_offs.tolist()] == three[1]
    text = piece * reps
    d_text = _dev(text)
    listed = sorted(tab.values())
    for unit in ("byte", "char"):
        e_ids, e_offs = _periodic(model, tab, piece, reps, unit)
        ids, offs = gv.encode_special_tensor(d_text, special_ids=listed, offsets=unit, copy=False)
        assert np.array_equal(_np(ids), e_ids) and np.array_equal(_np(offs), e_offs), unit
        assert gv.special_stats() == dict(n_literals=2 * reps, n_ids=len(e_ids), n_rows=-1, n_listed=len(listed))
        # by lines: one row per piece, offsets relative to it
        r_ids, r_splits, r_offs = gv.encode_special_rows_tensor(d_text, None, special_ids=listed, offsets=unit, copy=False)
        one = S.encode_special(model, piece[:-1], tab, unit)
        assert np.array_equal(_np(r_ids), e_ids) and np.array_equal(_np(r_splits), np.arange(reps + 1, dtype=np.int64) * len(one[0]))
        assert np.array_equal(_np(r_offs), np.tile(np.asarray(one[1], np.uint32), (reps, 1)))
        assert gv.special_stats()["n_rows"] == reps and gv.stats()["rows_route"] == 1
    assert np.array_equal(_np(gv.encode_special_tensor(d_text, special_ids=listed)), e_ids)
    host = gv.encode_special(text, special_ids=listed, offsets="byte")
    e_ids, e_offs = _periodic(model, tab, piece, reps, "byte")
    assert np.array_equal(host[0], e_ids) and np.array_equal(host[1], e_offs)


@pytest.mark.gpu
def test_growing_and_shrinking_calls_on_one_handle_after_trim(model, tab):
    hv = W.Vocab(VOCAB)
    listed = sorted(tab.values())
    piece = b"ab [MASK] \xc3\xa9[a]\n"
    for reps in (1, 40, 3000, 2, 900, 1):
        text = piece * reps
        for unit in ("byte", "char"):
            e_ids, e_offs = _periodic(model, tab, piece, reps, unit)
            ids, offs = hv.encode_special(text, special_ids=listed, offsets=unit)
            assert np.array_equal(ids, e_ids) and np.array_equal(offs, e_offs), (reps, unit)
            r = hv.encode_special_rows(text=text, special_ids=listed, offsets=unit)
            assert np.array_equal(r[0], e_ids) and len(r[1]) == reps + 1
        if reps == 3000:
            hv.trim()
    assert hv.encode_special("[MASK]", special_ids=listed).tolist() == [4]


def debug_suite():
    """what test_bounds_checking_build runs in a process of its own, on the checked build with guard zones"""
    gv, model = W.Vocab(VOCAB), R.Model(VOCAB)
    tab = S.table(VOCAB, S.special_ids(VOCAB, LISTED))
    gv.encode("a b")
    assert gv.stats()["reserved0"] == 1, "not the bounds-checking build"
    gv.set_option(W.WP_OPT_ARENA_GUARD, 1)
    for t in EDGE_TEXTS:
        flat_check(gv, model, tab, t, t)
    assert gv.stats()["guard_zones"] > 0
    text, places = _edge_text()
    assert flat_check(gv, model, tab, text, "edges") == 24
    rows_check(gv, model, tab, ROW_DOCS, "rows")
    vocab = VOCAB + ["ab", "a"]
    rows_check(W.Vocab(vocab), R.Model(vocab), S.table(vocab, S.special_ids(vocab, LISTED)), ROW_DOCS, "per document", route=0)
    piece, reps = "é [MASK]ab [SEP] ab\n".encode(), 5000
    listed = sorted(tab.values())
    for unit in ("byte", "char"):
        e_ids, e_offs = _periodic(model, tab, piece, reps, unit)
        ids, offs = gv.encode_special(piece * reps, special_ids=listed, offsets=unit)
        assert np.array_equal(ids, e_ids) and np.array_equal(offs, e_offs)
        assert np.array_equal(gv.encode_special_rows(text=piece * reps, special_ids=listed, offsets=unit)[0], e_ids)


@pytest.mark.gpu
def test_bounds_checking_build(tmp_path):
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "special_dbg_run.py"
    script.write_text('''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
from test_gpu_special import debug_suite
debug_suite()
print("SPECIAL_DEBUG_OK")
''' % (os.path.dirname(PKG), HERE))
    env = dict(os.environ, WP_LIB=dbg)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "SPECIAL_DEBUG_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_result_feeds_pack_and_detokenize_gives_the_ids_back(gv, model, tab):
    import torch
    listed = sorted(tab.values())
    docs = ["[CLS] hello [MASK] a [SEP]", "[CLS] cafe [SEP]", "", "[CLS] hellos [SEP] ab [MASK2] [SEP]"]
    text, off = W.join_docs(docs)
    d_off = torch.as_tensor(np.asarray(off, np.int64)).to("cuda:0")
    ids, splits = gv.encode_special_rows_tensor(_dev(text), d_off, special_ids=listed, copy=False)  # (views: the pack has buffers of its own)
    exp = S.encode_special_rows(model, docs, tab)
    assert _np(ids).tolist() == exp[0] and _np(splits).tolist() == exp[1]
    out = gv.pack_sequences_tensor(ids, splits, max_len=16, pad_id=3)
    ref = gv.pack_sequences(np.asarray(exp[0], np.int32), np.asarray(exp[1], np.int64), max_len=16, pad_id=3)
    assert all(np.array_equal(_np(out[k]), ref[k]) for k in ref)
    assert _np(out["input_ids"])[0, :5].tolist() == [1, 15, 4, 8, 2]
    # the round trip of the two calls: detokenize without skip_ids writes the specials out, encode_special_rows reads them
    h_ids, h_splits = np.asarray(exp[0], np.int32), np.asarray(exp[1], np.int64)
    texts = gv.detokenize(h_ids, row_splits=h_splits, cleanup=False)
    assert texts[0] == "[CLS] hello [MASK] a [SEP]" and texts[3] == "[CLS] hellos [SEP] ab [MASK2] [SEP]"
    back = gv.encode_special_rows(docs=texts, special_ids=listed)
    assert back[0].tolist() == exp[0] and back[1].tolist() == exp[1]
    plain = gv.encode_rows(docs=texts)
    assert plain[0].tolist() != exp[0]  # (what the plain call makes of the same text)
