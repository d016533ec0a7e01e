"""Pure-Python restatement of the documents contract of include/wordpiece_amd.h (wp_linear_encode_rows /
wp_linear_encode_padded) on top of offsets_model.py: the rows of a batch are the per-document encode_with_offsets, the
rows of a text are its lines, a padded batch is built from the rows.  Also the same rows cut out of ONE encode of the
joined text, which is what the library's joined route computes.

Model(vocab) parses the vocabulary once, so a batch of thousands of rows costs one parse: the walk is offsets_model's
(tests/test_rows_model.py holds the two against each other)."""
import bisect

import offsets_model as M
from bruteforce import is_space, is_spacing


class Model:
    """offsets_model.encode_spans with the vocabulary tables built once (they do not depend on the text: the copy of
    a duplicate line that a match names is decided inside the vocabulary stream)."""

    def __init__(self, vocab):
        toks, self.unk = M._vocab(vocab)
        V = [1]  # S = text . V
        after = []
        for _, _, cps in toks:
            V += cps + [1]
            after.append(len(V))  # index in V of what follows the token's separator
        self.tail = V

        def greater(a, b):  # V[a:] > V[b:]
            while True:
                x, y = V[a:a + 64], V[b:b + 64]
                if x != y or not x:
                    return x > y
                a += 64
                b += 64

        self.table, self.copies = ({}, {}), {}
        for i, (pf, bad, cps) in enumerate(toks):
            if not bad:
                d = self.table[pf].setdefault(len(cps), {})
                k = tuple(cps)
                self.copies.setdefault((pf, k), []).append(i)
                if k not in d or greater(after[i], after[d[k]]):
                    d[k] = i
        self.end_copy = {}
        for (pf, k), c in self.copies.items():
            if len(c) > 1:  # offsets_model.at_end: the nearest copy behind the vocabulary stream's own start, else the last
                behind = [j for j in c if greater(after[j], 1)]
                key = lambda j: tuple(V[after[j]:after[j] + 4096])
                self.end_copy[(pf, k)] = min(behind, key=key) if behind else max(c, key=key)
        self.lens = tuple(sorted(self.table[0], reverse=True)), tuple(sorted(self.table[1], reverse=True))

    def encode_spans(self, text):
        text = text if isinstance(text, (bytes, bytearray)) else text.encode("utf8")
        t, starts = M.decode_with_starts(text)
        if len(text) == 0:
            return [], [], t, starts
        n, tail, table, lens = len(t), self.tail, self.table, self.lens

        def wp(p):
            return p == 0 or is_spacing(t[p]) or is_spacing(t[p - 1])

        def best(p, prefix):
            for L in lens[prefix]:
                seg = t[p:p + L]
                if len(seg) < L:
                    seg = (seg + tail)[:L]
                k = tuple(seg)
                b = table[prefix][L].get(k)
                if b is not None:
                    return (self.end_copy.get((prefix, k), b) if p + L == n else b), L
            return -1, 0

        ids, spans, p, tsp = [], [], 0, 0
        while p != n and is_space(t[p]):
            p += 1
        while p < n:
            b, bl = best(p, 1 if wp(p) else 0)
            if b != -1:
                tsp += 1
                ids.append(b)
                spans.append((p, p + bl))
                p += bl
                if p < n and wp(p):
                    tsp = 0
            else:
                begin = spans[len(spans) - tsp][0] if tsp else p
                del ids[len(ids) - tsp:]
                del spans[len(spans) - tsp:]
                tsp = 0
                p += 1
                while p < n and not wp(p):
                    p += 1
                ids.append(self.unk)
                spans.append((begin, p))
            while p < n and is_space(t[p]):
                p += 1
        return ids, spans, t, starts

    def encode_with_offsets(self, text, unit="byte"):
        text = text if isinstance(text, (bytes, bytearray)) else text.encode("utf8")
        ids, spans, _, starts = self.encode_spans(text)
        return ids, (M.to_bytes(spans, text, starts) if unit == "byte" else spans)


def _b(d):
    return d if isinstance(d, (bytes, bytearray)) else d.encode("utf8")


def join_docs(docs):
    """-> (joined text, starts [n_docs + 1])"""
    docs = [_b(d) for d in docs]
    starts = [0]
    for d in docs:
        starts.append(starts[-1] + len(d) + 1)
    return b"".join(d + b"\n" for d in docs), starts


def split_lines(text):
    """The rows of lines mode: a text that does not end in a newline has a last line that runs to the end, one that
    does has no extra empty row."""
    parts = _b(text).split(b"\n")
    if parts[-1] == b"":
        parts.pop()
    return parts


def encode_rows(model, docs, unit=None):
    """The contract: -> (ids, row_splits, offsets or None), row i = model.encode_with_offsets(docs[i])"""
    ids, splits, offs = [], [0], []
    for d in docs:
        i, o = model.encode_with_offsets(_b(d), unit or "byte")
        ids += i
        offs += o
        splits.append(len(ids))
    return ids, splits, (offs if unit else None)


def encode_rows_joined(model, docs, unit=None):
    """The same from one encode of the joined text: an id belongs to the last document that starts at or before its span,
    offsets are taken relative to that start (in code points: to its first code point)."""
    text, dstart = join_docs(docs)
    ids, spans, t, starts = model.encode_spans(text)
    bspans = M.to_bytes(spans, text, starts)
    begins = [b for b, _ in bspans]
    splits = [bisect.bisect_left(begins, s) for s in dstart]
    if not unit:
        return ids, splits, None
    offs = []
    for r in range(len(docs)):
        base = dstart[r] if unit == "byte" else bisect.bisect_left(starts, dstart[r])
        src = bspans if unit == "byte" else spans
        offs += [(b - base, e - base) for b, e in src[splits[r]:splits[r + 1]]]
    return ids, splits, offs


def pack(ids, row_splits, max_len, cls_id=None, sep_id=None, pad_id=0):
    """-> (input_ids rows, lengths, rows that lost ids)"""
    head = [] if cls_id is None else [cls_id]
    tail = [] if sep_id is None else [sep_id]
    specials = len(head) + len(tail)
    assert max_len >= 1 and max_len >= specials
    rows, lengths, cut = [], [], 0
    for r in range(len(row_splits) - 1):
        T = ids[row_splits[r]:row_splits[r + 1]]
        keep = min(len(T), max_len - specials)
        cut += keep < len(T)
        row = head + list(T[:keep]) + tail
        lengths.append(len(row))
        rows.append(row + [pad_id] * (max_len - len(row)))
    return rows, lengths, cut
