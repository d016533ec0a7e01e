"""The contract of the detokenize calls (include/wordpiece_amd.h, section "detokenize") in plain Python: the two forms
of every id, the clean-up chain, rows in both layouts, the statistics — and the same in numpy for the sized case.

A vocabulary is a list of lines (bytes or str) and the set of its malformed ids; `Model.from_vocab` takes both from a
wordpiece_amd.Vocab (token_utf8 + token_flags), so that the line is what the library stores, not what the file said."""
import numpy as np

CHAIN = [(b" .", b"."), (b" ?", b"?"), (b" !", b"!"), (b" ,", b","), (b" ' ", b"'"), (b" n't", b"n't"), (b" 'm", b"'m"),
         (b" do not", b" don't"), (b" 's", b"'s"), (b" 've", b"'ve"), (b" 're", b"'re")]


def cleanup(s):
    """tokenizers.decoders.WordPiece(cleanup=True) on one token's string, over bytes."""
    for a, b in CHAIN:
        s = s.replace(a, b)
    return s


def piece(line, form, clean):
    """form0 = C(line); form1 = C(line without its leading "##") for a continuation token, C(" " + line) otherwise."""
    if form == 0:
        s = line
    elif line.startswith(b"##"):
        s = line[2:]
    else:
        s = b" " + line
    return cleanup(s) if clean else s


class Model:
    def __init__(self, lines, malformed=()):
        self.lines = [l.encode("utf-8") if isinstance(l, str) else bytes(l) for l in lines]
        self.malformed = frozenset(int(i) for i in malformed)
        self._tables = {}

    @classmethod
    def from_vocab(cls, v):
        lines, bad = [], []
        for i in range(len(v)):
            f = v.token_flags(i)
            lines.append(v.token_utf8(i) if f & 1 else b"##" + v.token_utf8(i))
            if f & 4:
                bad.append(i)
        return cls(lines, bad)

    def __len__(self):
        return len(self.lines)

    def piece(self, i, form, clean=True):
        if not 0 <= i < len(self.lines) or i in self.malformed or form not in (0, 1):
            return None
        return piece(self.lines[i], form, clean)

    def _rows(self, ids, row_splits, lengths):
        a = np.asarray(ids, dtype=np.int64)
        if a.ndim == 2:
            n_rows, max_len = a.shape
            lens = np.full(n_rows, max_len) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64), 0, max_len)
            return [a[r, :lens[r]] for r in range(n_rows)]
        splits = [0, len(a)] if row_splits is None else [int(x) for x in row_splits]
        assert splits[0] == 0 and all(x <= y for x, y in zip(splits, splits[1:]))
        return [a[splits[r]:splits[r + 1]] for r in range(len(splits) - 1)]

    def detokenize(self, ids, row_splits=None, lengths=None, skip_ids=(), clean=True, terminator=None):
        """-> (text bytes, text_off list of n_rows + 1, stats dict)"""
        skip = set(int(i) for i in skip_ids)
        term = b"" if terminator is None else (terminator.encode() if isinstance(terminator, str) else
                                                terminator if isinstance(terminator, bytes) else bytes([terminator]))
        out, off = [], [0]
        stats = {"n_rows": 0, "n_cells": 0, "n_kept": 0, "n_skipped": 0, "n_dropped": 0, "n_bytes": 0}
        at = 0
        for row in self._rows(ids, row_splits, lengths):
            first = True
            for x in row:
                x = int(x)
                stats["n_cells"] += 1
                if x < 0 or x >= len(self.lines) or x in self.malformed:
                    stats["n_dropped"] += 1
                elif x in skip:
                    stats["n_skipped"] += 1
                else:
                    stats["n_kept"] += 1
                    p = piece(self.lines[x], 0 if first else 1, clean)
                    first = False
                    out.append(p)
                    at += len(p)
            out.append(term)
            at += len(term)
            off.append(at)
            stats["n_rows"] += 1
        stats["n_bytes"] = at
        return b"".join(out), off, stats

    def strings(self, ids, **kw):
        text, off, _ = self.detokenize(ids, **kw)
        t = 0 if kw.get("terminator") is None else 1
        return [text[off[r]:off[r + 1] - t] for r in range(len(off) - 1)]

    # ---- the same in numpy, for ragged rows at size ---------------------------------------------------------------
    def _table(self, clean):
        """pool bytes, and offset / length indexed by (form, id); malformed ids have length 0 and are never kept"""
        if clean not in self._tables:
            V = len(self.lines)
            off = np.zeros((2, V), dtype=np.int64)
            ln = np.zeros((2, V), dtype=np.int64)
            pool = []
            at = 0
            for form in (0, 1):
                for i in range(V):
                    p = b"" if i in self.malformed else piece(self.lines[i], form, clean)
                    off[form, i], ln[form, i] = at, len(p)
                    pool.append(p)
                    at += len(p)
            self._tables[clean] = (np.frombuffer(b"".join(pool), dtype=np.uint8), off, ln)
        return self._tables[clean]

    def detokenize_np(self, ids, row_splits, skip_ids=(), clean=True, terminator=None):
        """Ragged rows, vectorised: a length table indexed by (form, id), a cumsum and a repeat-gather.
        -> (text uint8 array, text_off int64 array, stats dict)"""
        pool, off, ln = self._table(clean)
        V = len(self.lines)
        a = np.asarray(ids, dtype=np.int64)
        splits = np.asarray(row_splits, dtype=np.int64)
        n_rows, n = len(splits) - 1, len(a)
        bad = np.zeros(V, dtype=bool)
        bad[list(self.malformed)] = True
        in_range = (a >= 0) & (a < V)
        safe = np.where(in_range, a, 0)
        dropped = ~in_range | bad[safe]
        skipped = ~dropped & np.isin(a, np.asarray(list(skip_ids), dtype=np.int64))
        kept = ~dropped & ~skipped
        row = np.repeat(np.arange(n_rows), np.diff(splits))
        # kept cells in front of the cell, in its own row: 0 for the first kept cell of the row
        before = np.cumsum(kept) - kept
        kept_before_row = np.concatenate([[0], np.cumsum(kept)])[splits[:-1]]
        form = ((before - kept_before_row[row]) > 0).astype(np.int64)
        k_ids, k_form, k_row = safe[kept], form[kept], row[kept]
        k_len, k_off = ln[k_form, k_ids], off[k_form, k_ids]
        t = 0 if terminator is None else 1
        row_bytes = np.bincount(k_row, weights=k_len, minlength=n_rows).astype(np.int64) + t
        text_off = np.concatenate([[0], np.cumsum(row_bytes)]).astype(np.int64)
        total = int(text_off[-1])
        text = np.zeros(total, dtype=np.uint8)
        # where every kept piece starts: the pieces in front of it + one terminator per earlier row
        start = np.cumsum(k_len) - k_len + k_row * t
        which = np.repeat(np.arange(len(k_len)), k_len)
        within = np.arange(int(k_len.sum())) - np.repeat(np.cumsum(k_len) - k_len, k_len)
        text[start[which] + within] = pool[k_off[which] + within]
        if t:
            tb = terminator if isinstance(terminator, int) else (terminator.encode() if isinstance(terminator, str) else terminator)[0]
            text[text_off[1:] - 1] = tb
        stats = {"n_rows": n_rows, "n_cells": n, "n_kept": int(kept.sum()), "n_skipped": int(skipped.sum()),
                 "n_dropped": int(dropped.sum()), "n_bytes": total}
        return text, text_off, stats
