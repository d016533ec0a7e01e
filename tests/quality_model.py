"""Pure-Python restatement of the quality signals and rules (include/wordpiece_amd.h, section "quality signals"),
literal from the contract: every row on its own, characters by the decoder's rule with every uncovered byte a character
without a class, the word rule of the word counts per row, lines as maximal runs of bytes other than 0x0A, the 23
signals, the 16 rules as integer inequalities, the kept rows."""
import bisect
import re
import unicodedata

import count_model as CM
import offsets_model as OM

SIGNALS = ("bytes", "chars", "invalid", "space_chars", "alpha_chars", "digit_chars", "upper_chars", "punct_chars", "words", "text_words",
           "text_word_chars", "alpha_words", "stop_words", "hashes", "ellipses", "newlines", "lines", "bullet_lines", "ellipsis_lines",
           "terminal_lines", "short_lines", "dup_lines", "dup_line_chars")
RULES = ("min_text_words", "max_text_words", "min_mean_word_x1000", "max_mean_word_x1000", "max_hash_per_word", "max_ellipsis_per_word",
         "max_bullet_lines", "max_ellipsis_lines", "min_alpha_words", "min_stop_words", "max_dup_lines", "max_dup_line_chars",
         "min_terminal_lines", "max_short_lines", "max_newlines_per_word", "reserved")
S = {name: k for k, name in enumerate(SIGNALS)}
ELLIPSIS, BULLET = 0x2026, 0x2022
TERMINAL = tuple(b".!?\"'")


def characters(row):
    """-> [(byte start, bytes, code point or None)]: the decoder's characters and, one each, the bytes it drops"""
    cps, starts = OM.decode_with_starts(row)
    out, covered = [], bytearray(len(row))
    for cp, s in zip(cps, starts):
        n = OM.seq_len(row[s])
        covered[s:s + n] = b"\x01" * n
        out.append((s, n, cp))
    out += [(p, 1, None) for p in range(len(row)) if not covered[p]]
    return sorted(out)


def is_space(c):
    return c is not None and CM.is_space(c)


def is_punct(c):
    return c is not None and CM.is_punctuation(c)


def spacing(c):
    return c is not None and CM.spacing(c)


def category(c):
    return "" if c is None else unicodedata.category(chr(c))


def words_of(chars):
    """-> the words as lists of characters (the rule of the word counts, the row's first character for the text's)"""
    words = []
    for p, ch in enumerate(chars):
        c = ch[2]
        if is_space(c):
            continue
        start = p == 0 or spacing(c) or spacing(chars[p - 1][2])
        if start:
            words.append([ch])
        else:
            words[-1].append(ch)
    return words


def lines_of(row):
    """-> [(begin, end)] of the maximal runs of bytes other than 0x0A"""
    out, p = [], 0
    for piece in row.split(b"\n"):
        if piece:
            out.append((p, p + len(piece)))
        p += len(piece) + 1
    return out


def fold(b):
    return bytes(x + 32 if 65 <= x <= 90 else x for x in b)


def signals_of_row(row, stop_words=(), short_line_chars=30, dup_lines=True):
    row = bytes(row)
    short_line_chars = 30 if short_line_chars == 0 else short_line_chars
    chars = characters(row)
    s = [0] * len(SIGNALS)
    s[S["bytes"]] = len(row)
    s[S["chars"]] = len(chars)
    s[S["invalid"]] = sum(1 for c in chars if c[2] is None)
    s[S["space_chars"]] = sum(1 for c in chars if is_space(c[2]))
    s[S["alpha_chars"]] = sum(1 for c in chars if category(c[2])[:1] == "L")
    s[S["digit_chars"]] = sum(1 for c in chars if category(c[2]) == "Nd")
    s[S["upper_chars"]] = sum(1 for c in chars if category(c[2]) == "Lu")
    s[S["punct_chars"]] = sum(1 for c in chars if is_punct(c[2]))
    words = words_of(chars)
    stop = set(bytes(w) for w in stop_words)
    s[S["words"]] = len(words)
    text_words = [w for w in words if not is_punct(w[0][2])]
    s[S["text_words"]] = len(text_words)
    s[S["text_word_chars"]] = sum(len(w) for w in text_words)
    s[S["alpha_words"]] = sum(1 for w in words if any(category(c[2])[:1] == "L" for c in w))
    s[S["stop_words"]] = sum(1 for w in words if fold(row[w[0][0]:w[-1][0] + w[-1][1]]) in stop)
    s[S["hashes"]] = row.count(b"#")
    s[S["ellipses"]] = sum(1 for c in chars if c[2] == ELLIPSIS) + len(re.findall(rb"\.{3,}", row))
    s[S["newlines"]] = row.count(b"\n")
    lines = lines_of(row)
    s[S["lines"]] = len(lines)
    seen = set()
    char_starts = [c[0] for c in chars]
    for b, e in lines:
        inside = chars[bisect.bisect_left(char_starts, b):bisect.bisect_left(char_starts, e)]  # (the characters that start in [b, e))
        solid = [c for c in inside if not is_space(c[2])]
        if solid:
            first, last = solid[0], solid[-1]
            if first[2] in (ord("-"), BULLET):
                s[S["bullet_lines"]] += 1
            if last[2] == ELLIPSIS or (last[2] == ord(".") and last[0] - 2 >= b and row[last[0] - 2:last[0]] == b".."):
                s[S["ellipsis_lines"]] += 1
            if last[2] in TERMINAL:
                s[S["terminal_lines"]] += 1
        if len(inside) <= short_line_chars:
            s[S["short_lines"]] += 1
        if dup_lines:
            if row[b:e] in seen:
                s[S["dup_lines"]] += 1
                s[S["dup_line_chars"]] += len(inside)
            seen.add(row[b:e])
    return s


def reasons_of(s, limit):
    """the bitmask of the rules a row with the signals s fails (limit: 16 entries, -1: off)"""
    g = lambda name: s[S[name]]

    def ratio_over(num, den, L):
        return g(num) * 1000 > L * g(den)

    def ratio_under(num, den, L):
        return g(num) * 1000 < L * g(den)
    fails = (
        lambda L: g("text_words") < L,
        lambda L: g("text_words") > L,
        lambda L: ratio_under("text_word_chars", "text_words", L),
        lambda L: ratio_over("text_word_chars", "text_words", L),
        lambda L: ratio_over("hashes", "words", L),
        lambda L: ratio_over("ellipses", "words", L),
        lambda L: ratio_over("bullet_lines", "lines", L),
        lambda L: ratio_over("ellipsis_lines", "lines", L),
        lambda L: ratio_under("alpha_words", "words", L),
        lambda L: g("stop_words") < L,
        lambda L: ratio_over("dup_lines", "lines", L),
        lambda L: ratio_over("dup_line_chars", "chars", L),
        lambda L: ratio_under("terminal_lines", "lines", L),
        lambda L: ratio_over("short_lines", "lines", L),
        lambda L: ratio_over("newlines", "words", L),
    )
    r = 0
    for k, f in enumerate(fails):
        if limit[k] >= 0 and f(limit[k]):
            r |= 1 << k
    return r


def limits(**rules):
    out = [-1] * len(RULES)
    for name, v in rules.items():
        out[RULES.index(name)] = int(v)
    return out


GOPHER_STOP_WORDS = (b"the", b"be", b"to", b"of", b"and", b"that", b"have", b"with")
PRESETS = {
    "gopher": dict(limit=limits(min_text_words=50, max_text_words=100000, min_mean_word_x1000=3000, max_mean_word_x1000=10000, max_hash_per_word=100,
                                max_ellipsis_per_word=100, max_bullet_lines=900, max_ellipsis_lines=300, min_alpha_words=800, min_stop_words=2,
                                max_dup_lines=300, max_dup_line_chars=200), stop_words=GOPHER_STOP_WORDS),
    "fineweb": dict(limit=limits(min_terminal_lines=120, max_short_lines=670, max_dup_line_chars=10, max_newlines_per_word=300), stop_words=()),
}


def quality(data, row_off, limit=None, stop_words=(), short_line_chars=30, dup_lines=True):
    """-> dict(signals=[23][n_rows], reasons=[n_rows], kept=[rows], data=bytes, row_off=[...], stats=dict)"""
    data = bytes(data)
    limit = [-1] * len(RULES) if limit is None else list(limit)
    n = len(row_off) - 1
    rows = [data[row_off[i]:row_off[i + 1]] for i in range(n)]
    per_row = [signals_of_row(r, stop_words, short_line_chars, dup_lines) for r in rows]
    reasons = [reasons_of(s, limit) for s in per_row]
    kept = [i for i in range(n) if reasons[i] == 0]
    off = [0]
    for i in kept:
        off.append(off[-1] + len(rows[i]))
    total = lambda name: sum(s[S[name]] for s in per_row)
    stats = dict(n_rows=n, n_bytes=total("bytes"), n_chars=total("chars"), n_invalid=total("invalid"), n_words=total("words"), n_lines=total("lines"),
                 n_dup_lines=total("dup_lines"), n_kept=len(kept), rule_failed=[sum(1 for r in reasons if r >> k & 1) for k in range(len(RULES))])
    return dict(signals=[[s[k] for s in per_row] for k in range(len(SIGNALS))], reasons=reasons, kept=kept, data=b"".join(rows[i] for i in kept),
                row_off=off, stats=stats)
