"""Pure-Python restatement of the word counts (include/wordpiece_amd.h, section "word counts"): the normalised text of
normalize_model, the word rule of the walk on the vocabulary-independent classes, collections.Counter, the
two orders, max_word_bytes, min_count, the terminator and word_index."""
from collections import Counter

import normalize_model as NM
import offsets_model as OM

SPACE_TOKEN = 0x2581


def is_space(c):
    return (0x09 <= c <= 0x0D) or c == 0x20 or c == SPACE_TOKEN


def is_punctuation(c):
    if c < 256 and (0x21 <= c <= 0x2F or 0x3A <= c <= 0x40 or 0x5B <= c <= 0x60 or 0x7B <= c <= 0x7E):
        return True
    return c in (183, 171, 187, 8249, 8250) or 8208 <= c <= 8248


def is_chinese(c):
    return (0x4E00 <= c <= 0x9FFF or 0x3400 <= c <= 0x4DBF or 0x20000 <= c <= 0x2A6DF or 0x2A700 <= c <= 0x2B73F
            or 0x2B740 <= c <= 0x2B81F or 0x2B820 <= c <= 0x2CEAF or 0xF900 <= c <= 0xFAFF or 0x2F800 <= c <= 0x2FA1F)


def spacing(c):
    return is_space(c) or is_punctuation(c) or is_chinese(c)


def split(text, flags=0):
    """-> the words of the normalised text, as bytes, in text order (the rule of the header, literally)"""
    norm = NM.normalize(text, flags)[0]
    cps, starts = OM.decode_with_starts(norm)
    starts = list(starts) + [len(norm)]
    n = len(cps)
    is_start = [not is_space(cps[p]) and (p == 0 or spacing(cps[p]) or spacing(cps[p - 1])) for p in range(n)]
    words = []
    p = 0
    while p < n:
        if not is_start[p]:
            p += 1
            continue
        q = p + 1
        while q < n and not is_start[q] and not is_space(cps[q]):
            q += 1
        words.append(norm[starts[p]:starts[q]])
        p = q
    return words


def table(words, order="first", min_count=1, max_word_bytes=256, terminator=None, hash_bits=0):
    """words: what split() gives -> dict(words=[bytes], counts=[int], pool=bytes, word_off=[int], word_index=[int], stats)"""
    del hash_bits  # (never changes a result)
    min_count = 1 if min_count == 0 else min_count
    max_word_bytes = 256 if max_word_bytes == 0 else max_word_bytes
    listed = [w for w in words if len(w) <= max_word_bytes]
    cnt = Counter(listed)
    pairs = cnt.most_common() if order == "count" else list(cnt.items())
    kept = [(w, c) for w, c in pairs if c >= min_count]
    slot = {w: k for k, (w, _) in enumerate(kept)}
    term = b"" if terminator is None else bytes([terminator if isinstance(terminator, int) else terminator.encode()[0]])
    pool, off = b"", [0]
    for w, _ in kept:
        pool += w + term
        off.append(len(pool))
    stats = dict(n_words=len(words), n_distinct=len(kept), n_long=len(words) - len(listed), n_below_min=len(pairs) - len(kept),
                 n_text_bytes=None)
    return dict(words=[w for w, _ in kept], counts=[c for _, c in kept], pool=pool, word_off=off,
                word_index=[slot.get(w, -1) if len(w) <= max_word_bytes else -1 for w in words], stats=stats)


def count_words(text, flags=0, **kw):
    t = table(split(text, flags), **kw)
    t["stats"]["n_text_bytes"] = len(NM.normalize(text, flags)[0])
    return t
