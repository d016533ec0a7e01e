"""Pure-Python restatement of WP_OPT_NORMALIZE (include/wordpiece_amd.h): the rule per code point over the standard
library's unicodedata, on bytes (invalid UTF-8 dropped by the decode of offsets_model), and the offsets of an encode of
the normalised text carried back to the text the caller passed."""
import unicodedata as U

import offsets_model as OM

CLEAN, LOWER, STRIP = 1, 2, 4
FLAG_SETS = (1, 2, 3, 4, 5, 6, 7)


def normalize_cp(flags, c):
    """the code points code point c gives (clean, lower, strip, in that order)"""
    s = chr(c)
    if flags & CLEAN:
        cat = U.category(s)
        if c == 0 or c == 0xFFFD or (cat in ("Cc", "Cf") and c not in (0x09, 0x0A, 0x0D)):
            return []
        if cat == "Zs":
            s = " "
    if flags & LOWER:
        s = s.lower()
    if flags & STRIP:
        s = "".join(x for x in U.normalize("NFD", s) if U.category(x) != "Mn")
    return [ord(x) for x in s]


def normalize(text, flags, cache=None):
    """-> (normalised bytes, per normalised code point: source byte, source code-point index)"""
    text = text if isinstance(text, (bytes, bytearray)) else text.encode("utf8")
    cps, starts = OM.decode_with_starts(text)
    cache = {} if cache is None else cache
    out, src_byte, src_cp = [], [], []
    for i, c in enumerate(cps):
        img = cache.get(c)
        if img is None:
            img = cache[c] = normalize_cp(flags, c)
        for x in img:
            out.append(chr(x))
            src_byte.append(starts[i])
            src_cp.append(i)
    return "".join(out).encode("utf8", "surrogatepass"), src_byte, src_cp


def carry_spans(spans, text, src_byte, src_cp, unit):
    """spans [b, e) in normalised code points -> the caller's text: from the start of the source code point of b to
    the end of the source code point of e - 1"""
    if unit == "char":
        return [(src_cp[b], src_cp[e - 1] + 1) for b, e in spans]
    return [(src_byte[b], src_byte[e - 1] + OM.seq_len(text[src_byte[e - 1]])) for b, e in spans]


def encode_spans_normalized(text, vocab, flags, unit="byte"):
    """-> (ids, [(begin, end)] in the text the caller passed) as Vocab(vocab, normalize=flags).encode_with_offsets"""
    text = text if isinstance(text, (bytes, bytearray)) else text.encode("utf8")
    norm, src_byte, src_cp = normalize(text, flags)
    ids, spans, _, _ = OM.encode_spans(norm, vocab)
    return ids, carry_spans(spans, text, src_byte, src_cp, unit)
