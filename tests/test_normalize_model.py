"""tests/normalize_model.py (the rule of WP_OPT_NORMALIZE, one code point at a time) against the whole-string
formulation of BERT's BasicTokenizer: _clean_text, str.lower(), NFD + drop Mn."""
import random
import unicodedata as U

import normalize_model as NM

# the 23 combining marks that are not Mn: whole-string NFD reorders them by class, the rule does not (documented)
NON_MN_COMBINING = frozenset(c for c in range(0x110000) if U.combining(chr(c)) and U.category(chr(c)) != "Mn")


def clean_text(s):
    """BERT's _clean_text — except that U+0009 / U+000A / U+000D stay as they are instead of becoming U+0020 (they are
    blanks for the walk either way, and the documents calls find their rows by U+000A)."""
    out = []
    for ch in s:
        c = ord(ch)
        cat = U.category(ch)
        if c in (0x09, 0x0A, 0x0D):
            out.append(ch)
        elif c == 0 or c == 0xFFFD or cat in ("Cc", "Cf"):
            continue
        elif cat == "Zs":
            out.append(" ")
        else:
            out.append(ch)
    return "".join(out)


def run_strip_accents(s):
    return "".join(ch for ch in U.normalize("NFD", s) if U.category(ch) != "Mn")


def whole_string(s, flags):
    if flags & NM.CLEAN:
        s = clean_text(s)
    if flags & NM.LOWER:
        s = s.lower()
    if flags & NM.STRIP:
        s = run_strip_accents(s)
    return s


def _alphabet():
    cps = list(range(0x0000, 0x3000)) + list(range(0xAC00, 0xAC00 + 11172)) + list(range(0x1D100, 0x1D200))
    return [c for c in cps if c != 0x3A3 and c not in NON_MN_COMBINING and not 0xD800 <= c < 0xE000]


def test_there_are_23_combining_marks_outside_mn():
    if U.unidata_version == "13.0.0":
        assert len(NON_MN_COMBINING) == 23
    assert 0x1D165 in NON_MN_COMBINING and 0x302E in NON_MN_COMBINING and 0x1B44 in NON_MN_COMBINING


def test_model_equals_the_whole_string_formulation():
    rng = random.Random(20240613)
    alphabet = _alphabet()
    hot = [c for c in alphabet if c < 0x250 or 0x300 <= c < 0x370]  # Latin with accents and combining marks, often
    cache = {f: {} for f in NM.FLAG_SETS}
    for k in range(20000):
        n = rng.randint(0, 24)
        s = "".join(chr(rng.choice(hot if rng.random() < 0.5 else alphabet)) for _ in range(n))
        flags = NM.FLAG_SETS[k % 7] if k % 3 else 7
        got, src_byte, src_cp = NM.normalize(s.encode("utf8"), flags, cache[flags])
        assert got.decode("utf8") == whole_string(s, flags), (flags, [hex(ord(c)) for c in s])
        assert len(src_byte) == len(src_cp) == len(got.decode("utf8"))
        assert src_cp == sorted(src_cp) and all(0 <= q < len(s) for q in src_cp)


def test_the_two_documented_differences():
    # no final sigma: the rule looks at one code point
    assert NM.normalize("ΟΔΟΣ".encode(), 7)[0].decode() == "οδοσ" and whole_string("ΟΔΟΣ", 7) == "οδος"
    # neighbouring combining marks that are not Mn are not reordered by class (216 before 226 in whole-string NFD)
    pair = "\U0001D16D\U0001D165"
    assert NM.normalize(pair.encode(), 4)[0].decode() == pair and whole_string(pair, 4) == "\U0001D165\U0001D16D"


def test_invalid_bytes_are_dropped_and_sources_kept():
    text = b"A\xffB\xcc\x81\xe4\xb8" + "É".encode() + b"\xc3"
    got, src_byte, src_cp = NM.normalize(text, 7)
    assert got == b"abe" and src_byte == [0, 2, 7] and src_cp == [0, 1, 3]
    ids, spans = NM.encode_spans_normalized(text, [b"[UNK]", b"abe"], 7, "byte")
    assert ids == [1] and spans == [(0, 9)]
    ids, spans = NM.encode_spans_normalized(text, [b"[UNK]", b"abe"], 7, "char")
    assert ids == [1] and spans == [(0, 4)]


def test_spans_go_back_to_the_callers_text():
    vocab = [b"[UNK]", b"hello", b"cafe", b"##s", b"world"]
    text = "Hello CAFÉS wor​ld"
    ids, spans = NM.encode_spans_normalized(text, vocab, 7, "char")
    assert ids == [1, 2, 3, 4] and spans == [(0, 5), (6, 10), (10, 11), (12, 18)]
    ids, spans = NM.encode_spans_normalized(text, vocab, 7, "byte")
    assert spans == [(0, 5), (7, 12), (12, 13), (14, 22)]
    # a Hangul syllable is one source code point however many jamo it gives (the vocabulary holds the jamo: it is not normalised)
    ids, spans = NM.encode_spans_normalized("\uac01\u00e1".encode(), [b"[UNK]", "\u1100\u1161\u11a8a".encode()], 7, "char")
    assert ids == [1] and spans == [(0, 2)]
