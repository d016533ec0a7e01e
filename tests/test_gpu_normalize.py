"""WP_OPT_NORMALIZE on the GPU: the pre-pass alone against the model (tests/normalize_model.py), ids against an encode of
the model-normalised text on the same GPU, offsets of both units against encode_spans_normalized, the documents calls
against encode_with_offsets(document), the option switched off again, and the sharded / pipelined entry points."""
import json
import os
import random

import numpy as np
import pytest

import normalize_model as NM
import offsets_model as M
import wordpiece_amd as W
from wordpiece_amd import synth
from test_gpu_offsets import _medium_cases

HERE = os.path.dirname(os.path.abspath(__file__))
FLAG_SETS = NM.FLAG_SETS
_CACHES = {f: {} for f in FLAG_SETS}


def _model(text, flags):
    return NM.normalize(text, flags, _CACHES[flags])


# ---- inputs ----------------------------------------------------------------------------------------------------------
_PIECES = (["a", "b", "c", "é", "ж", "中", "文", "\U0001F600", "-", ",", " ", "\t", "▁", "\n"] +
           ["A", "B", "C", "É", "Ж", "e\u0301", "E\u0300\u0323", "ç", "Å", "ǆ", "Ω", "Σ", "ς", "я", "Й", "ё", "İ", "ı", "ß",
            "각", "가", "힣", "한", "ᄀ", "﨑", "\u00a0", "\u2003", "\u3000", "\u1680", "\u200b", "\u200d", "\ufeff", "\u00ad",
            "\u0000", "\u0001", "\u000b", "\u000c", "\r", "\u007f", "\u0085", "\ufffd", "\U000E0001", "\U0001D165", "\u0301"])
_INVALID = [b"\xff", b"\xc3", b"\xe4\xb8", b"\x80", b"\xf0\x9f", b"\xed\xa0\x80", b"\xc0\xaf", b"\xf4\x90\x80\x80"]
_BORDERS = (1023, 1024, 1025, 16383, 16384, 16385)


def random_text(rng, k):
    """Small texts of every kind of code point the rule treats; every 20th case is 17-40 KB with invalid bytes and
    truncated sequences at row and tile borders and at the end, and runs of combining marks (one longer than a tile)."""
    parts = []
    for _ in range(rng.randint(0, 40)):
        r = rng.random()
        if r < 0.06:
            parts.append(rng.choice(_INVALID))
        elif r < 0.10:
            parts.append((rng.choice(["e", "A", "가"]) + rng.choice(["\u0301", "\u20d0", "\u0323"]) * rng.randint(1, 12)).encode())
        else:
            parts.append(rng.choice(_PIECES).encode())
    text = b"".join(parts)
    if k % 20 == 0:
        words = [rng.choice(["Hello", "wörld", "ÀÉÎ", "naïve", "한국어", "ΚΑΛΗΜΕΡΑ", "Привет", "中文", "abc", "İstanbul"])
                 for _ in range(rng.randint(2500, 6000))]
        big = bytearray(rng.choice([" ", "\u00a0", "\n", " \u200b"]).join(words).encode())
        run = rng.choice([1, 7, 300, 2000, 9000])
        at = rng.randrange(0, len(big))
        while at < len(big) and big[at] & 0xC0 == 0x80:
            at += 1
        big[at:at] = ("e" + rng.choice(["\u0301", "\u20d0"]) * run + "x").encode()
        for pos in _BORDERS:
            if pos + 4 < len(big) and rng.random() < 0.8:
                cut = rng.choice(_INVALID + ["é".encode(), "中".encode(), "\U0001F600".encode(), "힣".encode()])
                big[pos - rng.randint(0, len(cut) - 1):pos + 1] = cut  # a sequence that straddles, or breaks at, the border
        text = bytes(big) + text + rng.choice([b"", b"\xe4\xb8", b"\xc3", b"\xf0\x9f\x98", "É".encode(), b"\xff"])
    return text


def random_cases(n=1000, seed=17):
    rng = random.Random(seed)
    out = []
    for k in range(n):
        _, vocab = M.random_case(rng)
        if k % 3 == 0:  # tokens only the normalised text can match
            vocab = vocab + [w for w in (b"hello", b"world", b"##e", b"e", "각".encode(), "ᄀ".encode(), "##ᅡ".encode(),
                                         "привет".encode(), b"istanbul", b"i") if w not in vocab]
        out.append((random_text(rng, k), vocab))
    return out


_ACCENT = {ord("a"): "àáâä", ord("e"): "èéêë", ord("i"): "ìíîï", ord("o"): "òóôö", ord("u"): "ùúûü", ord("c"): "ç", ord("n"): "ñ"}


def decorate(text, seed):
    """A seeded transform of a lower-case text that flags 7 undo: ASCII letters upper-cased or accented (precomposed, or
    with a combining mark behind them), blanks turned into U+00A0, zero-width spaces put inside words; other scripts get
    combining marks and zero-width spaces only."""
    rng = random.Random(seed)
    out = bytearray()
    wide = False  # the code point in front is not ASCII (CJK, Cyrillic: a mark or a zero-width space behind some of them)
    for b in text:
        r = rng.random()
        if wide and b & 0xC0 != 0x80 and r < 0.04:
            out += ("\u0301" if r < 0.02 else "\u200b").encode()
            r = 1.0
        if b & 0xC0 != 0x80:
            wide = b >= 0xC0
        if 0x61 <= b <= 0x7A and r < 0.30:
            if r < 0.04 and b in _ACCENT:
                ch = rng.choice(_ACCENT[b])
                out += (ch.upper() if r < 0.02 else ch).encode()
            elif r < 0.06:
                out += bytes([b]) + "\u0301".encode()
            elif r < 0.08:
                out += bytes([b]) + "\u200b".encode()
            else:
                out.append(b - 0x20)
        elif b == 0x20 and r < 0.05:
            out += "\u00a0".encode()
        else:
            out.append(b)
    return bytes(out)


def golden_cases():
    out = []
    for name in ("reference_tests_cpp.json", "survey_probed_cases.json"):
        with open(os.path.join(HERE, "golden", name)) as f:
            for case in json.load(f)["cases"]:
                out.append((bytes.fromhex(case["text_hex"]), [bytes.fromhex(w) for w in case["vocab_hex"]]))
    return out


# ---- a vectorised form of the model for texts of 1-3-byte code points (the 64 MB case) --------------------------------
def _bmp_table(flags):
    n = np.zeros(0x10000, dtype=np.int32)
    img = np.zeros((0x10000, 3), dtype=np.int32)
    for c in range(0x10000):
        if 0xD800 <= c < 0xE000:
            continue
        o = NM.normalize_cp(flags, c)
        n[c] = len(o)
        img[c, :len(o)] = o
    return n, img


def _utf8_encode_np(cps):
    ln = np.where(cps < 0x80, 1, np.where(cps < 0x800, 2, 3))
    start = np.cumsum(ln) - ln
    out = np.zeros(int(ln.sum()), dtype=np.uint8)
    one, two, three = ln == 1, ln == 2, ln == 3
    out[start[one]] = cps[one]
    out[start[two]] = 0xC0 | (cps[two] >> 6)
    out[start[two] + 1] = 0x80 | (cps[two] & 0x3F)
    out[start[three]] = 0xE0 | (cps[three] >> 12)
    out[start[three] + 1] = 0x80 | ((cps[three] >> 6) & 0x3F)
    out[start[three] + 2] = 0x80 | (cps[three] & 0x3F)
    return out


def numpy_decode(text):
    """valid UTF-8 of 1-3-byte sequences -> (code points, their first bytes)"""
    tb = np.frombuffer(text, dtype=np.uint8).astype(np.int32)
    starts = np.nonzero((tb & 0xC0) != 0x80)[0]
    lead = tb[starts]
    pad = np.concatenate([tb, np.zeros(2, dtype=np.int32)])
    b1, b2 = pad[starts + 1] & 0x3F, pad[starts + 2] & 0x3F
    cps = np.where(lead < 0x80, lead, np.where(lead < 0xE0, ((lead & 0x1F) << 6) | b1, ((lead & 0x0F) << 12) | (b1 << 6) | b2))
    assert (lead < 0xF0).all()
    return cps, starts


def numpy_normalize(text, table):
    n, img = table
    cps, _ = numpy_decode(text)
    cnt = n[cps]
    src = np.repeat(np.arange(len(cps)), cnt)
    within = np.arange(len(src)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return _utf8_encode_np(img[cps[src], within]).tobytes(), src


def mixed_case_english(nbytes, seed):
    """English-shaped text, upper case at a third of the word starts, 1 % of the words accented"""
    text, vocab = synth.english_corpus(nbytes, seed=seed, vocab_size=8000)
    tb = np.frombuffer(text, dtype=np.uint8).copy()
    rng = np.random.default_rng(seed)
    word_start = np.nonzero((tb >= 0x61) & (tb <= 0x7A) & (np.concatenate([[0x20], tb[:-1]]) == 0x20))[0]
    tb[word_start[rng.random(len(word_start)) < 0.33]] -= 0x20
    acc = word_start[rng.random(len(word_start)) < 0.01] + 1  # the second letter of the word, when it is one we have an accent for
    acc = acc[acc < len(tb)]
    acc = acc[np.isin(tb[acc], np.frombuffer(b"aeiou", dtype=np.uint8))]
    second = {0x61: 0xA1, 0x65: 0xA9, 0x69: 0xAD, 0x6F: 0xB3, 0x75: 0xBA}  # á é í ó ú = C3 xx
    ins = np.array([second[int(x)] for x in tb[acc]], dtype=np.uint8)
    tb[acc] = 0xC3
    out = np.insert(tb, acc + 1, ins)
    return out.tobytes(), vocab


# ---- the stage alone -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_stage_alone_random_texts():
    gv = W.Vocab(["[UNK]", "a"], device=0)
    cases = random_cases()
    assert sum(len(t) > 16500 for t, _ in cases) >= 40
    for k, (text, _) in enumerate(cases):
        for f in FLAG_SETS:
            assert gv.normalize(text, flags=f) == _model(text, f)[0], (k, f, len(text))
    # no flags: the valid sequences, copied
    for text, _ in cases[:100]:
        assert gv.normalize(text, flags=0) == "".join(map(chr, M.decode_with_starts(text)[0])).encode("utf8")


@pytest.mark.gpu
def test_rows_that_grow_by_more_than_three_times_their_size():
    """A code point belongs to the row (1 KB of source) that holds its lead byte, so a row of 3-byte Hangul LVT
    syllables that starts on a syllable holds 342 leads and gives 342 * 9 = 3078 bytes, more than 3 * 1024; the 4-byte
    musical symbols U+1D15E..U+1D164 (2-3 code points of 4 bytes each) do the same from row phase 3.  Every row phase,
    texts of many rows, against the model; then ids and offsets through such rows."""
    gv = W.Vocab(["[UNK]", "a"], device=0)
    lvt = "".join(chr(0xAC01 + 28 * (i % 300) + i % 27) for i in range(6000))  # LVT syllables only: 3 jamo each
    assert all((ord(c) - 0xAC00) % 28 for c in lvt)
    notes = "".join(chr(0x1D15E + i % 7) for i in range(3000))
    for body in (lvt, "\uac01" * 400, notes, lvt[:700] + notes[:600] + lvt[:900]):
        for phase in range(5):
            text = ("x" * phase + body + "y").encode()
            for f in FLAG_SETS:
                assert gv.normalize(text, flags=f) == _model(text, f)[0], (phase, f, len(text))
    jamo = [b"[UNK]", b"a"] + [chr(c).encode() for c in range(0x1100, 0x1113)] + [("##" + chr(c)).encode() for c in range(0x1100, 0x11C3)]
    text = ("a " + lvt[:1500] + " " + lvt[1500:2600]).encode()
    _ids_and_offsets_check(jamo, text, 7, "hangul rows")
    _ids_and_offsets_check(jamo, text, 4, "hangul rows")


@pytest.mark.gpu
def test_stage_alone_64mb_and_tensor():
    import torch
    text, _ = mixed_case_english(64 << 20, seed=21)
    assert len(text) >= 64 << 20
    head = text[:5000].decode("utf8", "ignore")
    assert any(c.isupper() for c in head) and any(ord(c) > 0x7F for c in text[:200000].decode("utf8", "ignore"))
    gv = W.Vocab(["[UNK]", "a"], device=0)
    t = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    for f in FLAG_SETS:
        table = _bmp_table(f)
        sample = text[1 << 20:(1 << 20) + 30000].decode("utf8", "ignore").encode()
        assert numpy_normalize(sample, table)[0] == _model(sample, f)[0]  # the vectorised form is the model
        exp = np.frombuffer(numpy_normalize(text, table)[0], dtype=np.uint8)
        got = np.frombuffer(gv.normalize(text, flags=f), dtype=np.uint8)
        assert np.array_equal(got, exp), f
        if f in (1, 7):
            assert np.array_equal(gv.normalize_tensor(t, flags=f).cpu().numpy(), exp), f


# ---- ids and offsets -------------------------------------------------------------------------------------------------
def _ids_and_offsets_check(vocab, text, f, label, plain=None, offsets=True):
    """ids == the plain handle's ids of the model-normalised text; offsets of both units == encode_spans_normalized"""
    gv = W.Vocab(vocab, normalize=f)
    plain = plain or W.Vocab(vocab)
    norm = _model(text, f)[0]
    exp = plain.encode(norm)
    got = gv.encode(text)
    assert np.array_equal(got, exp), (label, f)
    if text:
        st = gv.stats()
        assert st["normalize"] == f and st["norm_bytes"] == len(norm) and st["n_bytes"] == len(text), (label, f)
    if offsets:
        for unit in ("byte", "char"):
            exp_ids, exp_spans = NM.encode_spans_normalized(text, vocab, f, unit)
            ids, offs = gv.encode_with_offsets(text, unit=unit)
            assert ids.tolist() == exp_ids == exp.tolist(), (label, f, unit)
            assert [tuple(r) for r in offs.tolist()] == exp_spans, (label, f, unit)
    return gv, got


@pytest.mark.gpu
def test_pinned_example():
    vocab = ["[UNK]", "hello", "cafe", "##s", "world"]
    text = "Hello\u00a0CAFÉS wor\u200bld"
    assert W.Vocab(vocab).encode(text).tolist() == [0, 0]
    gv = W.Vocab(vocab, normalize=W.WP_NORM_BERT_UNCASED)
    assert gv.encode(text).tolist() == [1, 2, 3, 4] and gv.fast_encode(text).tolist() == [1, 2, 3, 4]
    assert gv.normalize(text) == b"hello cafes world"
    ids, offs = gv.encode_with_offsets(text, unit="char")
    assert ids.tolist() == [1, 2, 3, 4] and offs.tolist() == [[0, 5], [6, 10], [10, 11], [12, 18]]
    ids, offs = gv.encode_with_offsets(text, unit="byte")
    assert offs.tolist() == [[0, 5], [7, 12], [12, 13], [14, 22]]
    assert W.Vocab(vocab, normalize=W.WP_NORM_CLEAN).encode(text).tolist() == [0, 0, 4]  # cased BERT: split, not lowered
    # a text the rule leaves nothing of; a Hangul syllable is one source code point
    assert len(gv.encode("\u200b\u0301\ufeff")) == 0 and gv.stats()["norm_bytes"] == 0
    gv = W.Vocab(["[UNK]", "\u1100\u1161\u11a8a"], normalize=7)  # (the vocabulary is not normalised: it holds the jamo)
    ids, offs = gv.encode_with_offsets("\uac01\u00e1", unit="char")
    assert ids.tolist() == [1] and offs.tolist() == [[0, 2]]


@pytest.mark.gpu
def test_golden_and_random_cases_every_flag_set():
    n = 0
    for text, vocab in golden_cases():
        try:
            plain = W.Vocab(vocab)
        except W.WordPieceError:
            continue
        for f in FLAG_SETS:
            _ids_and_offsets_check(vocab, text, f, "golden", plain)
            _ids_and_offsets_check(vocab, decorate(text, n), f, "golden, decorated", plain)
        n += 1
    assert n > 10
    changed = 0
    for k, (text, vocab) in enumerate(random_cases()):
        plain = W.Vocab(vocab)
        f = FLAG_SETS[k % 7]
        for flags in ((f, 7) if f != 7 else (7,)):
            _, got = _ids_and_offsets_check(vocab, text, flags, "random %d" % k, plain)
        changed += not np.array_equal(got, plain.encode(text))
    assert changed > 300  # the rule matters on these texts


@pytest.mark.gpu
def test_medium_inputs_on_every_walk_path():
    for j, (label, text, vocab, opts, want) in enumerate(_medium_cases()):
        deco = decorate(text, 100 + j)
        plain = W.Vocab(vocab)
        for k, v in opts.items():
            plain.set_option(k, v)
        base = plain.encode(deco)
        for f in FLAG_SETS:
            gv = W.Vocab(vocab, normalize=f)
            for k, v in opts.items():
                gv.set_option(k, v)
            norm, src_byte, src_cp = _model(deco, f)
            exp = plain.encode(norm)
            got = gv.encode(deco)
            assert np.array_equal(got, exp), (label, f)
            if f == 7 and len(exp) > 1:  # (other flag sets leave part of the decoration: a word may fail with and without
                # them; the single word that is built to fail is one missing id either way)
                assert not np.array_equal(got, base), (label, "the un-normalised encode gives the same ids")
            if f == 7 and norm == _model(text, 7)[0]:  # the decoration undone: the walk takes the path the case was built for
                st = gv.stats()
                for key, val in want.items():
                    assert st[key] == val, (label, key, st[key])
            exp_ids, spans, _, _ = M.encode_spans(norm, vocab)
            assert exp_ids == exp.tolist(), (label, f)
            for unit in ("byte", "char"):
                ids, offs = gv.encode_with_offsets(deco, unit=unit)
                assert ids.tolist() == exp_ids, (label, f, unit)
                assert [tuple(r) for r in offs.tolist()] == NM.carry_spans(spans, deco, src_byte, src_cp, unit), (label, f, unit)
            if label in ("staged class rule", "coverage rule"):
                assert np.array_equal(gv.fast_encode(deco), plain.fast_encode(norm)), (label, f)


@pytest.mark.gpu
def test_fast_path():
    for k, (text, vocab) in enumerate(random_cases(300, seed=5)):
        plain = W.Vocab(vocab)
        for f in (FLAG_SETS[k % 7], 7):
            assert np.array_equal(W.Vocab(vocab, normalize=f).fast_encode(text), plain.fast_encode(_model(text, f)[0])), (k, f)


@pytest.mark.gpu
def test_full_size_promises():
    """64 MB, flags 7: ids of the normalised text; spans increasing and disjoint; char and byte units agree through the
    source's code-point starts; every source code point that is kept and not a blank lies in exactly one span"""
    text, vocab = mixed_case_english(64 << 20, seed=22)
    text = decorate(text[:1 << 20], 9) + text[1 << 20:]  # (combining marks, U+00A0 and zero-width spaces in the first MB)
    table = _bmp_table(7)
    norm, src = numpy_normalize(text, table)
    gv = W.Vocab(vocab, normalize=7, device=0)
    plain = W.Vocab(vocab, device=0)
    exp = plain.encode(norm)
    assert np.array_equal(gv.encode(text), exp) and not np.array_equal(plain.encode(text), exp)
    ids, ob = gv.encode_with_offsets(text, unit="byte")
    ids_c, oc = gv.encode_with_offsets(text, unit="char")
    assert np.array_equal(ids, exp) and np.array_equal(ids_c, exp)
    b, e = ob[:, 0].astype(np.int64), ob[:, 1].astype(np.int64)
    assert (b < e).all() and (b[1:] >= e[:-1]).all() and e[-1] <= len(text)
    cps, starts = numpy_decode(text)
    cb, ce = oc[:, 0].astype(np.int64), oc[:, 1].astype(np.int64)
    assert (cb < ce).all() and (cb[1:] >= ce[:-1]).all() and ce[-1] <= len(cps)
    tb = np.frombuffer(text, dtype=np.uint8)
    last = starts[ce - 1]
    seq = np.where(tb[last] < 0x80, 1, np.where(tb[last] < 0xE0, 2, 3))
    assert np.array_equal(starts[cb], b) and np.array_equal(last + seq, e)
    # the spans are those of the plain encode of the normalised text, carried back
    _, on = plain.encode_with_offsets(norm, unit="char")
    assert np.array_equal(src[on[:, 0].astype(np.int64)], cb) and np.array_equal(src[on[:, 1].astype(np.int64) - 1] + 1, ce)
    d = np.zeros(len(cps) + 1, dtype=np.int32)
    np.add.at(d, cb, 1)
    np.add.at(d, ce, -1)
    cover = np.cumsum(d)[:len(cps)]
    assert cover.max() == 1
    n, img = table
    kept = n[cps] > 0
    blank = np.isin(img[cps, 0], [9, 10, 11, 12, 13, 32, 0x2581]) & (n[cps] == 1)
    assert (cover[kept & ~blank] == 1).all()


# ---- documents -------------------------------------------------------------------------------------------------------
_DOCS = ["Hello\u00a0CAFÉS wor\u200bld", "", "\ufeffHello", "\u200b\u0301", "CAFÉ\u0301s\u200b", "  héllo  ", "\u00a0", "각 Hello\u0000World",
         "a\nHELLO\n\u00adb", "wor\u00adld\ufeff", "İstanbul ΣΟΦΊΑ hello" * 3]


def _lines(t):
    return t.split(b"\n")[:-1] if t.endswith(b"\n") else t.split(b"\n")


def _rows_check(vocab, f, docs, route):
    gv = W.Vocab(vocab, normalize=f)
    text, off = W.join_docs(docs)
    per_doc = {}
    for unit in ("byte", "char"):
        per_doc[unit] = [gv.encode_with_offsets(d, unit=unit) for d in docs]
    lines = _lines(text)
    open_end = text + "\u200b\ufeff".encode()  # a last line the rule leaves nothing of: still a row
    for mode, t, o, rows in (("explicit", text, off, [W._bytes(d) for d in docs]), ("lines", text, None, lines),
                             ("lines, open end", open_end, None, lines + ["\u200b\ufeff".encode()]),
                             ("lines, open", text[:-1], None, _lines(text[:-1]))):
        for unit in (None, "byte", "char"):
            got = gv.encode_rows(text=t, doc_offsets=o, offsets=unit)
            assert gv.stats()["rows_route"] == route and gv.stats()["normalize"] == f, (mode, unit)
            ids, splits = got[0], got[1]
            assert len(splits) == len(rows) + 1 and splits[0] == 0 and splits[-1] == len(ids), (f, mode, unit)
            for i, d in enumerate(rows):
                e_ids, e_offs = gv.encode_with_offsets(d, unit=unit or "char")
                assert ids[splits[i]:splits[i + 1]].tolist() == e_ids.tolist(), (f, mode, unit, i)
                if unit:
                    assert got[2][splits[i]:splits[i + 1]].tolist() == e_offs.tolist(), (f, mode, unit, i)
    # padded batches against the rows
    ids, splits = gv.encode_rows(docs=docs)
    for max_len, cls, sep in ((6, 101, 102), (3, None, None), (16, 7, None)):
        pid, plen = gv.encode_padded(docs=docs, max_len=max_len, cls_id=cls, sep_id=sep, pad_id=9)
        head = [] if cls is None else [cls]
        tail = [] if sep is None else [sep]
        for i in range(len(docs)):
            row = ids[splits[i]:splits[i + 1]].tolist()[:max_len - len(head) - len(tail)]
            want = head + row + tail
            assert plen[i] == len(want) and pid[i].tolist() == want + [9] * (max_len - len(want)), (f, i, max_len)
    return gv, text, off, ids, splits


@pytest.mark.gpu
def test_documents_both_routes():
    import torch
    vocab = ["[UNK]", "hello", "cafe", "##s", "world", "a", "b", "##b", "istanbul", "σοφια", "각", "ᄀ", "##ᅡ", "##ᆨ", "i", "##\u0307"]
    rng = random.Random(3)
    more = [t.decode("utf8", "ignore").replace("\n", " ") for t, _ in random_cases(60, seed=9) if len(t) < 300]
    for f in FLAG_SETS:
        docs = _DOCS + more[(f - 1) * 8:(f - 1) * 8 + 8]
        rng.shuffle(docs)
        for v, route in ((vocab, 1), (vocab + ["hello"], 0)):  # a duplicate eligible line: one encode per document
            gv, text, off, ids, splits = _rows_check(v, f, docs, route)
            if f in (1, 7):  # the tensor forms
                t = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
                o = torch.from_numpy(off).to("cuda:0")
                ti, ts, to = gv.encode_rows_tensor(t, o, offsets="byte")
                e_ids, e_splits, e_offs = gv.encode_rows(text=text, doc_offsets=off, offsets="byte")
                assert np.array_equal(ti.cpu().numpy(), e_ids) and np.array_equal(ts.cpu().numpy(), e_splits)
                assert np.array_equal(to.view(torch.int32).cpu().numpy().view(np.uint32), e_offs)
                pid, plen = gv.encode_padded_tensor(t, o, max_len=8, cls_id=101, sep_id=102)
                hid, hlen = gv.encode_padded(text=text, doc_offsets=off, max_len=8, cls_id=101, sep_id=102)
                assert np.array_equal(pid.cpu().numpy(), hid) and np.array_equal(plen.cpu().numpy(), hlen)
                pid, plen = gv.encode_padded_tensor(t, None, max_len=8, cls_id=101, sep_id=102)
                hid, hlen = gv.encode_padded(text=text, max_len=8, cls_id=101, sep_id=102)
                assert np.array_equal(pid.cpu().numpy(), hid) and np.array_equal(plen.cpu().numpy(), hlen)
    with pytest.raises(W.WordPieceError, match="document offsets"):  # checked on the caller's text
        W.Vocab(vocab, normalize=7).encode_rows_tensor(torch.frombuffer(bytearray("Aé\nb\n".encode()), dtype=torch.uint8).to("cuda:0"),
                                                       torch.tensor([0, 3, 5], dtype=torch.int64, device="cuda:0"))


@pytest.mark.gpu
def test_documents_medium():
    """a few thousand decorated lines through the joined route against the per-document encode of the same handle"""
    text, vocab = synth.english_corpus(400_000, seed=31, vocab_size=3000)
    words = decorate(text.replace(b"\n", b" "), 5).split(b" ")
    rng = random.Random(4)
    docs, i = [], 0
    while i < len(words):
        k = rng.choice([0, 1, 3, 9, 40])
        docs.append(b" ".join(words[i:i + k]) + rng.choice([b"", b"", "\u200b".encode(), "\ufeff ".encode()]))
        i += k
    for f in (1, 6, 7):
        gv = W.Vocab(vocab + ["[UNK]"], normalize=f)
        t, off = W.join_docs(docs)
        for unit in ("byte", "char"):
            ids, splits, offs = gv.encode_rows(text=t, doc_offsets=off, offsets=unit)
            assert gv.stats()["rows_route"] == 1
            l_ids, l_splits, l_offs = gv.encode_rows(text=t, offsets=unit)
            assert np.array_equal(ids, l_ids) and np.array_equal(splits, l_splits) and np.array_equal(offs, l_offs)
            whole = gv.encode(t)
            assert np.array_equal(ids, whole)
            for j in rng.sample(range(len(docs)), 150):
                e_ids, e_offs = gv.encode_with_offsets(docs[j], unit=unit)
                assert np.array_equal(ids[splits[j]:splits[j + 1]], e_ids), (f, unit, j)
                assert np.array_equal(offs[splits[j]:splits[j + 1]], e_offs.reshape(-1, 2)), (f, unit, j)


# ---- the option off again; sharded and pipelined calls ---------------------------------------------------------------
_TIMINGS = ("ms_total", "ms_decode", "ms_sa", "ms_lcp", "ms_scan", "ms_walk", "ms_radix_scatter", "ms_h2d", "ms_d2h", "ms_host_total",
            "ms_normalize")


@pytest.mark.gpu
def test_option_off_again_is_a_fresh_handle():
    text, vocab = synth.english_corpus(2 << 20, seed=8, vocab_size=6000)
    deco = decorate(text, 3)
    fresh = W.Vocab(vocab, device=0)
    exp = fresh.encode(deco)
    st_fresh = fresh.stats()
    assert st_fresh["normalize"] == 0 and st_fresh["norm_bytes"] == 0 and st_fresh["ms_normalize"] == 0.0
    gv = W.Vocab(vocab, device=0)
    gv.set_option(W.WP_OPT_NORMALIZE, 7)
    on = gv.encode(deco)
    norm = _model(deco, 7)[0]
    assert gv.stats()["normalize"] == 7 and gv.stats()["norm_bytes"] == len(norm) and np.array_equal(on, fresh.encode(norm))
    gv.set_option(W.WP_OPT_NORMALIZE, 0)
    off = gv.encode(deco)
    st = gv.stats()
    assert np.array_equal(off, exp) and not np.array_equal(off, on)
    # Every field but the timings — and but arena_bytes and list_retries, which no two handles of a process share: they
    # follow the memory of the handle's context (arenas that only grow, the list room of its last encode), and a new
    # handle takes over the context some destroyed handle parked, with that memory (include/wordpiece_amd.h, wp_trim).
    for k in st:
        if k not in _TIMINGS and k not in ("arena_bytes", "list_retries"):
            assert st[k] == st_fresh[k], k
    gv.set_option(W.WP_OPT_STAGE_TIMING, 1)
    gv.set_option(W.WP_OPT_NORMALIZE, 7)
    gv.encode(deco)
    st = gv.stats()
    assert 0.0 < st["ms_normalize"] < st["ms_total"]


@pytest.mark.gpu
def test_multi_and_batch():
    text, vocab = synth.english_corpus(6 << 20, seed=9, vocab_size=6000)
    deco = decorate(text[:1 << 20], 2) + "\u000b".encode() + mixed_case_english(5 << 20, seed=9)[0]
    for f in (1, 7):
        gv = W.Vocab(vocab, normalize=f, device=0)
        single = gv.encode(deco)
        multi = gv.encode_multi(deco, devices=[0, 0])
        assert gv.stats()["n_devices"] == 2 and gv.stats()["normalize"] == f
        assert np.array_equal(multi, single), f
        cut = deco.index(b" ", len(deco) // 3)
        cut2 = deco.index(b" ", 2 * len(deco) // 3)
        parts = [deco[:cut], b"", deco[cut:cut2], deco[cut2:]]
        got = gv.encode_batch(parts)
        assert np.array_equal(np.concatenate(got), single), f
        for p, g in zip(parts, got):
            assert np.array_equal(g, gv.encode(p))
