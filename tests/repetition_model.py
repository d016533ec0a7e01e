"""Pure-Python restatement of the repetition signals and rules (include/wordpiece_amd_repetition.h), literal from the
contract: the words of quality_model per row, n-grams as tuples of word bytes, a Counter for the most frequent 2- to
4-grams, a dict of first positions for the duplicated 5- to 10-grams, the nine rules as integer inequalities."""
from collections import Counter

import quality_model as Q

SIGNALS = ("words", "word_chars", "top_2_count", "top_2_chars", "top_3_count", "top_3_chars", "top_4_count", "top_4_chars", "dup_5_chars",
           "dup_6_chars", "dup_7_chars", "dup_8_chars", "dup_9_chars", "dup_10_chars")
RULES = ("max_top_2_chars", "max_top_3_chars", "max_top_4_chars", "max_dup_5_chars", "max_dup_6_chars", "max_dup_7_chars", "max_dup_8_chars",
         "max_dup_9_chars", "max_dup_10_chars")
S = {name: k for k, name in enumerate(SIGNALS)}
GOPHER = dict(zip(RULES, (200, 180, 160, 150, 140, 130, 120, 110, 100)))


def words_of_row(row):
    """-> [(bytes of the word, its characters)]"""
    row = bytes(row)
    return [(row[w[0][0]:w[-1][0] + w[-1][1]], len(w)) for w in Q.words_of(Q.characters(row))]


def signals_of_row(row):
    words = words_of_row(row)
    text = [w[0] for w in words]
    chars = [w[1] for w in words]
    s = [0] * len(SIGNALS)
    s[S["words"]] = len(words)
    s[S["word_chars"]] = sum(chars)
    for n in (2, 3, 4):
        count = Counter()
        size = {}
        for p in range(len(words) - n + 1):
            g = tuple(text[p:p + n])
            count[g] += 1
            size[g] = sum(chars[p:p + n])
        best = max(((c, size[g]) for g, c in count.items()), default=(0, 0))  # (by occurrences, then by characters)
        if best[0] >= 2:
            s[S["top_%d_count" % n]] = best[0]
            s[S["top_%d_chars" % n]] = best[0] * best[1]
    for n in range(5, 11):
        seen = set()
        covered = [False] * len(words)
        for p in range(len(words) - n + 1):
            g = tuple(text[p:p + n])
            if g in seen:
                for j in range(p, p + n):
                    covered[j] = True
            seen.add(g)
        s[S["dup_%d_chars" % n]] = sum(c for c, x in zip(chars, covered) if x)
    return s


def reasons_of(s, limit):
    r = 0
    for k in range(len(RULES)):
        x = s[S["top_%d_chars" % (k + 2)]] if k < 3 else s[S["dup_%d_chars" % (k + 2)]]
        if limit[k] >= 0 and x * 1000 > limit[k] * s[S["word_chars"]]:
            r |= 1 << k
    return r


def limits(**rules):
    out = [-1] * len(RULES)
    for name, v in rules.items():
        out[RULES.index(name)] = int(v)
    return out


def repetition(data, row_off, limit=None):
    """-> dict(signals=[14][n_rows], reasons=[n_rows], kept=[rows], data=bytes, row_off=[...], stats=dict)"""
    data = bytes(data)
    limit = [-1] * len(RULES) if limit is None else list(limit)
    n = len(row_off) - 1
    rows = [data[row_off[i]:row_off[i + 1]] for i in range(n)]
    per_row = [signals_of_row(r) for r in rows]
    reasons = [reasons_of(s, limit) for s in per_row]
    kept = [i for i in range(n) if reasons[i] == 0]
    off = [0]
    for i in kept:
        off.append(off[-1] + len(rows[i]))
    stats = dict(n_rows=n, n_bytes=len(data[:row_off[n]]) if n else 0, n_words=sum(s[0] for s in per_row), n_word_chars=sum(s[1] for s in per_row),
                 n_kept=len(kept), rule_failed=[sum(1 for r in reasons if r >> k & 1) for k in range(len(RULES))])
    return dict(signals=[[s[k] for s in per_row] for k in range(len(SIGNALS))], reasons=reasons, kept=kept, data=b"".join(rows[i] for i in kept),
                row_off=off, stats=stats)
