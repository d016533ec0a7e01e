"""The contract of include/wordpiece_amd_bpe.h in executable form, standard library and numpy only: the classes from
unicodedata, the pieces by a plain sequential scan of the pattern's alternatives (NOT by the header's local rules 1-3, which
the device uses: the two are checked against each other), the merge loop one pair at a time (lowest rank, leftmost), and a
small seeded trainer that produces proper merge lists."""
import collections
import unicodedata as U

import numpy as np

SPACES = frozenset([0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680] + list(range(0x2000, 0x200B)) + [0x2028, 0x2029, 0x202F, 0x205F, 0x3000])
CONTRACTIONS = ("s", "t", "re", "ve", "m", "ll", "d")  # in the order of the pattern


def class_of(ch):
    if ord(ch) in SPACES:
        return "S"
    cat = U.category(ch)
    return cat[0] if cat[0] in "LN" else "O"


def chars(doc):
    """-> [(first byte, end, class, the character or None)]: a well-formed sequence is a character, any other byte one of class O"""
    out, i = [], 0
    while i < len(doc):
        b = doc[i]
        k = 1 if b < 0x80 else 2 if 0xC2 <= b <= 0xDF else 3 if 0xE0 <= b <= 0xEF else 4 if 0xF0 <= b <= 0xF4 else 0
        ch = None
        if k and i + k <= len(doc):
            try:
                ch = doc[i:i + k].decode("utf-8")
            except UnicodeDecodeError:
                pass
        if ch is None or len(ch) != 1:
            out.append((i, i + 1, "O", None))
            i += 1
        else:
            out.append((i, i + k, class_of(ch), ch))
            i += k
    return out


def pieces(doc):
    """the byte ranges of the pieces of one document: at every position the first alternative of the pattern that matches"""
    cs = chars(doc)
    n, K, CH = len(cs), [c[2] for c in cs], [c[3] for c in cs]

    def run(j, k):
        while j < n and K[j] == k:
            j += 1
        return j
    cuts, i = [], 0
    while i < n:
        e = None
        if CH[i] == "'":  # 's|'t|'re|'ve|'m|'ll|'d
            e = next((i + 1 + len(t) for t in CONTRACTIONS if [c for c in CH[i + 1:i + 1 + len(t)]] == list(t)), None)
        for k in "LNO" if e is None else "":  # ` ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+`
            if CH[i] == " " and i + 1 < n and K[i + 1] == k:
                e = run(i + 1, k)
            elif K[i] == k:
                e = run(i, k)
            if e is not None:
                break
        if e is None:  # `\s+(?!\S)|\s+`: the run without its last character where a non-space follows and the run has two
            r = run(i, "S")
            e = r if r == n or r - 1 == i else r - 1
        cuts.append((cs[i][0], cs[e - 1][1]))
        i = e
    return cuts


def bytes_to_unicode():
    keep = list(range(0x21, 0x7F)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    rest = [b for b in range(256) if b not in keep]
    return {**{b: chr(b) for b in keep}, **{b: chr(256 + k) for k, b in enumerate(rest)}}


class Model:
    """byte_id: 256 ids; merges: [(left, right, result)], the index the rank"""

    def __init__(self, byte_id, merges):
        self.byte_id, self.merges = [int(x) for x in byte_id], [tuple(int(x) for x in m) for m in merges]
        self.rank = {(l, r): (k, res) for k, (l, r, res) in enumerate(self.merges)}
        self.n_ids = max(self.byte_id + [m[2] for m in self.merges]) + 1

    def merge(self, piece):
        """-> [(id, bytes)]: one pair at a time, the lowest rank present, the leftmost of its occurrences"""
        sym = [(self.byte_id[b], 1) for b in piece]
        while True:
            found = [(self.rank[(sym[i][0], sym[i + 1][0])][0], i) for i in range(len(sym) - 1) if (sym[i][0], sym[i + 1][0]) in self.rank]
            if not found:
                return sym
            k, i = min(found)
            sym[i:i + 2] = [(self.merges[k][2], sym[i][1] + sym[i + 1][1])]

    def encode(self, docs):
        """what bpe_encode_rows returns with offsets and pieces, and "rounds": the merges of the piece that took the most"""
        ids, begin, end, row_splits, piece_splits, rounds = [], [], [], [0], [], 0
        for d in docs:
            for a, b in pieces(d):
                piece_splits.append(len(ids))
                at, syms = a, self.merge(d[a:b])
                rounds = max(rounds, (b - a) - len(syms))
                for i, ln in syms:
                    ids.append(i)
                    begin.append(at)
                    end.append(at + ln)
                    at += ln
            row_splits.append(len(ids))
        return dict(ids=np.array(ids, dtype=np.int32), row_splits=np.array(row_splits, dtype=np.int64), begin=np.array(begin, dtype=np.int32),
                    end=np.array(end, dtype=np.int32), piece_splits=np.array(piece_splits + [len(ids)], dtype=np.int64), rounds=rounds)

    def vocab(self):
        """-> ({token: id} in the byte-level alphabet, [(a, b)] the merges as token pairs): what bpe_load and `tokenizers` take"""
        alphabet = bytes_to_unicode()
        tok = {self.byte_id[b]: alphabet[b] for b in range(256)}
        pairs = []
        for l, r, res in self.merges:
            tok[res] = tok[l] + tok[r]
            pairs.append((tok[l], tok[r]))
        return {t: i for i, t in tok.items()}, pairs


def train(texts, n_merges, seed=0):
    """A proper merge list learnt from the pieces of `texts` (bytes): the byte ids are a seeded permutation of 0..255, merge
    k yields the new id 256 + k and joins the most frequent adjacent pair (the smallest pair on ties)."""
    byte_id = np.random.default_rng(seed).permutation(256).tolist()
    words = collections.Counter(tuple(byte_id[b] for b in t[a:e]) for t in texts for a, e in pieces(t))
    merges = []
    for k in range(n_merges):
        pairs = collections.Counter()
        for w, c in words.items():
            for p in zip(w, w[1:]):
                pairs[p] += c
        if not pairs:
            break
        (l, r), _ = min(pairs.items(), key=lambda kv: (-kv[1], kv[0]))
        merges.append((l, r, 256 + k))
        nxt = collections.Counter()
        for w, c in words.items():
            out, i = [], 0
            while i < len(w):
                if i + 1 < len(w) and (w[i], w[i + 1]) == (l, r):
                    out.append(256 + k)
                    i += 2
                else:
                    out.append(w[i])
                    i += 1
            nxt[tuple(out)] += c
        words = nxt
    return Model(byte_id, merges)
