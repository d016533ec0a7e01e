"""Pure-Python restatement of the special-tokens contract of include/wordpiece_amd.h (section "special tokens":
wp_linear_encode_special / wp_linear_encode_special_rows) on top of rows_model.Model: which vocabulary lines may be
listed, where their literals lie in a text, the blanked text, and the merge of the literals' ids into the encode of the
blanked text.  The documents form is defined per document.

What Hugging Face's BertTokenizer does with its added special tokens (split_special_tokens=False): the text is cut at
the literals before it is normalised, each literal becomes its id, everything between them is tokenized on its own
(tests/golden/special_tokenizers_cases.json holds the two against each other)."""
from bruteforce import is_punct

MAX_LITERAL = 64   # bytes of a line that may be listed
MAX_LISTED = 4096  # ids in a spec


def _b(x):
    return bytes(x) if isinstance(x, (bytes, bytearray, memoryview)) else x.encode("utf8")


def eligible_line(line):
    """May this vocabulary line be listed?  wp_vocab_token_flags bit 1 set (a "[...]" line of more than two code
    points) and bit 2 clear (not punctuation only), at most 64 bytes, every byte in 0x21..0x7E, '[' only first and
    ']' only last."""
    line = _b(line)
    if not (2 < len(line) <= MAX_LITERAL) or line[0] != 0x5B or line[-1] != 0x5D:
        return False
    inner = line[1:-1]
    if any(c < 0x21 or c > 0x7E or c == 0x5B or c == 0x5D for c in inner):
        return False
    return not all(is_punct(c) for c in inner)


def special_ids(vocab, tokens=None):
    """Vocab.special_ids: the ids of the given strings (first line that equals each), or of every eligible line (the
    first copy of a line that repeats: two listed ids may not share a line)."""
    lines = [_b(w) for w in vocab]
    if tokens is None:
        seen, out = set(), []
        for i, w in enumerate(lines):
            if eligible_line(w) and w not in seen:
                seen.add(w)
                out.append(i)
        return out
    return [lines.index(_b(t)) for t in tokens]


def table(vocab, ids):
    """{line: id} of a spec; ValueError(the offending id in the message) where the library gives WP_ERR_ARG."""
    lines = [_b(w) for w in vocab]
    if len(ids) > MAX_LISTED:
        raise ValueError("more than %d ids listed" % MAX_LISTED)
    tab = {}
    for i in ids:
        if not 0 <= i < len(lines):
            raise ValueError("id %d is out of range" % i)
        if not eligible_line(lines[i]):
            raise ValueError("id %d is no literal line" % i)
        if tab.get(lines[i], i) != i:
            raise ValueError("id %d repeats the line of id %d" % (i, tab[lines[i]]))
        tab[lines[i]] = i
    return tab


def find(text, tab):
    """The literals of a text, in order: [(byte start, length, id)].  At every '[' the candidate is the bytes up to and
    including the next ']': it matches when it ends inside the text, has at most 64 bytes, holds only 0x21..0x7E with no
    further '[', and equals a listed line.  Decided by the text alone, so two literals never overlap."""
    text = _b(text)
    out = []
    n = len(text)
    for p in range(n):
        if text[p] != 0x5B:
            continue
        q = p + 1
        while q < n and q - p < MAX_LITERAL and 0x21 <= text[q] <= 0x7E and text[q] not in (0x5B, 0x5D):
            q += 1
        if q < n and q - p < MAX_LITERAL and text[q] == 0x5D:
            i = tab.get(text[p:q + 1])
            if i is not None:
                out.append((p, q + 1 - p, i))
    return out


def blank(text, lits):
    b = bytearray(_b(text))
    for p, l, _ in lits:
        b[p:p + l] = b" " * l
    return bytes(b)


def _cp_before(text):
    """number of valid code points in front of every byte position (the decoder's verdicts)"""
    import offsets_model as M
    _, starts = M.decode_with_starts(text)
    pre = [0] * (len(text) + 1)
    for s in starts:
        pre[s + 1] = 1
    for i in range(len(text)):
        pre[i + 1] += pre[i]
    return pre


def encode_special(model, text, tab, unit=None):
    """The flat form -> (ids, offsets or None): the encode of the blanked text with (id, [start, end)) of every literal
    merged in by position, in bytes ("byte") or code points ("char") of the caller's text."""
    text = _b(text)
    lits = find(text, tab)
    ids, offs = model.encode_with_offsets(blank(text, lits), unit or "byte")
    if not lits:
        return list(ids), ([tuple(o) for o in offs] if unit else None)
    pre = _cp_before(text) if unit == "char" else None
    items = [(o[0], i, tuple(o)) for i, o in zip(ids, offs)]
    for p, l, i in lits:
        span = (p, p + l) if unit != "char" else (pre[p], pre[p] + l)
        items.append((span[0], i, span))
    items.sort(key=lambda x: x[0])  # (begins are distinct between a literal and a token: no span covers a blanked byte)
    return [x[1] for x in items], ([x[2] for x in items] if unit else None)


def encode_special_rows(model, docs, tab, unit=None):
    """The documents form -> (ids, row_splits, offsets or None): row i is the flat form of document i."""
    ids, splits, offs = [], [0], []
    for d in docs:
        i, o = encode_special(model, d, tab, unit)
        ids += i
        if unit:
            offs += o
        splits.append(len(ids))
    return ids, splits, (offs if unit else None)


def encode_segments(model, text, tab):
    """The same ids and byte offsets stated segment by segment: the stretches between literals encoded one by one, the
    literals' ids in between (what a tokenizer that cuts the text at its added tokens does)."""
    text = _b(text)
    ids, offs, at = [], [], 0
    for p, l, i in find(text, tab) + [(len(text), 0, None)]:
        si, so = model.encode_with_offsets(text[at:p], "byte")
        ids += si
        offs += [(b + at, e + at) for b, e in so]
        if i is not None:
            ids.append(i)
            offs.append((p, p + l))
        at = p + l
    return ids, offs
