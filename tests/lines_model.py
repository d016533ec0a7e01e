"""Pure-Python restatement of the line filter (include/wordpiece_amd_lines.h), literal from the contract: characters,
words and lines from tests/quality_model.py; phrases by a fold and a slice comparison at every position; duplicate lines
through a dict over the line bytes; the cut by joining what is not owned by a dropped line."""
import bisect
import itertools

import quality_model as Q

SIGNALS = ("bytes", "kept_bytes", "lines", "kept_lines", "line_chars", "kept_chars", "words", "kept_words", "failed_0", "failed_1", "failed_2", "failed_3",
           "failed_4", "failed_5", "doc_phrase_hits")
LINE_RULES = ("min_words", "min_chars", "not_terminal", "ellipsis_end", "phrase", "duplicate")
DOC_RULES = ("min_kept_lines", "min_kept_words", "max_dropped_x1000", "max_doc_phrase_hits")
S = {name: k for k, name in enumerate(SIGNALS)}
BOUNDED, DOC = 1, 2


def boundary(b):
    return b < 0x80 and not chr(b).isalnum()


def matches(row, p, phrase, flags):
    n = len(phrase)
    if Q.fold(row[p:p + n]) != phrase:  # (a slice cut by the row end is shorter: no match)
        return False
    return not flags & BOUNDED or ((p == 0 or boundary(row[p - 1])) and (p + n == len(row) or boundary(row[p + n])))


def lines_of_row(row, line_limit, phrases):
    """-> ([dict(begin, end, own, words, chars, reasons)] without the DUPLICATE bit, the document-phrase hits, all matches)"""
    chars = Q.characters(row)
    starts = [c[0] for c in chars]
    words = [(w[0][0], w[-1][0] + w[-1][1]) for w in Q.words_of(chars)]
    spans = Q.lines_of(row)
    out, doc_hits, line_hits = [], 0, 0
    for k, (b, e) in enumerate(spans):
        inside = chars[bisect.bisect_left(starts, b):bisect.bisect_left(starts, e)]
        solid = [c for c in inside if not Q.is_space(c[2])]
        n_words = sum(1 for s, _ in words if b <= s < e)
        last = solid[-1] if solid else None
        r = 0
        if 0 <= line_limit[0] and n_words < line_limit[0]:
            r |= 1
        if 0 <= line_limit[1] and len(inside) < line_limit[1]:
            r |= 2
        if 0 <= line_limit[2] and (last is None or last[2] not in Q.TERMINAL):
            r |= 4
        if 0 <= line_limit[3] and last is not None and (last[2] == Q.ELLIPSIS or (last[2] == ord(".") and last[0] - 2 >= b and row[last[0] - 2:last[0]] == b"..")):
            r |= 8
        for p in range(b, e):
            for phrase, flags in phrases:
                if matches(row, p, phrase, flags):
                    if flags & DOC:
                        doc_hits += 1
                    else:
                        r |= 16
                        line_hits += 1
        out.append(dict(begin=b, end=e, own=spans[k + 1][0] if k + 1 < len(spans) else len(row), words=n_words, chars=len(inside), reasons=r))
    return out, doc_hits, doc_hits + line_hits


def doc_reasons(s, doc_limit):
    g = lambda name: s[S[name]]
    fails = (lambda L: g("kept_lines") < L, lambda L: g("kept_words") < L, lambda L: (g("line_chars") - g("kept_chars")) * 1000 > L * g("line_chars"),
             lambda L: g("doc_phrase_hits") > L)
    return sum(1 << k for k, f in enumerate(fails) if doc_limit[k] >= 0 and f(doc_limit[k]))


def limits(**rules):
    line, doc = [-1] * 4, [-1] * 4
    for name, x in rules.items():
        if name in DOC_RULES:
            doc[DOC_RULES.index(name)] = int(x)
        else:
            line[LINE_RULES[:4].index(name)] = int(x)
    return line, doc


def filter_lines(data, row_off, rules=None, phrases=(), doc_phrases=(), bounded=False, dup_scope=0, dup_min_chars=0):
    """-> dict of every array of the call as lists / bytes, and stats"""
    data = bytes(data)
    line_limit, doc_limit = limits(**(rules or {}))
    flag = BOUNDED if bounded else 0
    enc = lambda p: p.encode() if isinstance(p, str) else bytes(p)
    plist = [(enc(p), flag) for p in phrases] + [(enc(p), flag | DOC) for p in doc_phrases]
    n = len(row_off) - 1
    seen, sig, reasons, lines, cut_rows, n_matches = set(), [], [], [], [], 0
    for i in range(n):
        row = data[row_off[i]:row_off[i + 1]]
        ls, doc_hits, hits = lines_of_row(row, line_limit, plist)
        n_matches += hits
        if dup_scope == 1:
            seen = set()
        s = [0] * len(SIGNALS)
        s[S["bytes"]], s[S["doc_phrase_hits"]], s[S["lines"]] = len(row), doc_hits, len(ls)
        keep = bytearray(b"\x01" * len(row))
        for ln in ls:
            text = row[ln["begin"]:ln["end"]]
            if dup_scope and text in seen and ln["chars"] >= dup_min_chars:
                ln["reasons"] |= 32
            seen.add(text)
            s[S["line_chars"]] += ln["chars"]
            s[S["words"]] += ln["words"]
            if ln["reasons"]:
                keep[ln["begin"]:ln["own"]] = bytes(ln["own"] - ln["begin"])
                for k in range(6):
                    s[S["failed_0"] + k] += ln["reasons"] >> k & 1
            else:
                s[S["kept_lines"]] += 1
                s[S["kept_chars"]] += ln["chars"]
                s[S["kept_words"]] += ln["words"]
            lines.append((i, row_off[i] + ln["begin"], ln["end"] - ln["begin"], ln["reasons"]))
        cut_rows.append(bytes(b for b, k in zip(row, keep) if k))
        s[S["kept_bytes"]] = len(cut_rows[-1])
        sig.append(s)
        reasons.append(doc_reasons(s, doc_limit))
    kept = [i for i in range(n) if reasons[i] == 0]
    offsets = lambda rows: list(itertools.accumulate((len(r) for r in rows), initial=0))
    total = lambda name: sum(s[S[name]] for s in sig)
    stats = dict(n_rows=n, n_bytes=total("bytes"), n_lines=len(lines), n_kept_lines=total("kept_lines"), n_kept_bytes=total("kept_bytes"), n_kept=len(kept),
                 line_failed=[total("failed_%d" % k) for k in range(6)], rule_failed=[sum(1 for r in reasons if r >> k & 1) for k in range(4)],
                 n_phrase_matches=n_matches)
    return dict(signals=[[s[k] for s in sig] for k in range(len(SIGNALS))], reasons=reasons, line_row=[x[0] for x in lines], line_start=[x[1] for x in lines],
                line_len=[x[2] for x in lines], line_reasons=[x[3] for x in lines], cut_data=b"".join(cut_rows), cut_off=offsets(cut_rows), kept=kept,
                data=b"".join(cut_rows[i] for i in kept), row_off=offsets([cut_rows[i] for i in kept]), stats=stats)
