"""Pure-Python restatement of the offsets semantics of wp_linear_encode_offsets (include/wordpiece_amd.h): the walk
of bruteforce.encode (linear.cpp:221-274), recording (id, begin, end) per id in code points, and the map to bytes.
Longest match through one dict of tokens per length, so texts of a few hundred KB stay cheap."""
from bruteforce import is_punct, is_space, is_spacing


def decode_with_starts(b):
    """bruteforce.decode that also keeps the byte start of every code point (same drop rule)."""
    out, starts, i, n = [], [], 0, len(b)
    while i < n:
        c = b[i]
        if c < 0x80:
            out.append(c)
            starts.append(i)
            i += 1
            continue
        need = 2 if c & 0xE0 == 0xC0 else 3 if c & 0xF0 == 0xE0 else 4 if c & 0xF8 == 0xF0 else 0
        ok = need and i + need <= n and all(b[i + k] & 0xC0 == 0x80 for k in range(1, need))
        if ok:
            cp = c & (0x1F if need == 2 else 0x0F if need == 3 else 0x07)
            for k in range(1, need):
                cp = (cp << 6) | (b[i + k] & 0x3F)
            lo = {2: 0x80, 3: 0x800, 4: 0x10000}[need]
            if cp >= lo and (cp < 0xD800 or 0xDFFF < cp < 0x110000):
                out.append(cp)
                starts.append(i)
                i += need
                continue
        i += 1
    return out, starts


def _vocab(vocab):
    """tokens as bruteforce.encode parses them: (prefix, unusable, cps); unk id"""
    toks, unk = [], -1
    for i, w in enumerate(vocab):
        w = w if isinstance(w, (bytes, bytearray)) else w.encode("utf8")
        if w == b"[UNK]":
            unk = i
        cps, _ = decode_with_starts(w)
        prefix, special = True, False
        if len(cps) >= 2 and cps[0] == 35 and cps[1] == 35:
            prefix, cps = False, cps[2:]
        elif len(cps) > 2 and cps[0] == 91 and cps[-1] == 93:
            special = True
        if not cps:
            raise RuntimeError("Vocab word is empty")
        malformed = len(cps) > 1 and all(is_punct(c) or is_space(c) for c in cps)
        toks.append((prefix, special or malformed, cps))
    return toks, unk


def encode_spans(text, vocab):
    """-> (ids, spans in code points [(begin, end)], code points, byte starts of the code points)"""
    text = text if isinstance(text, (bytes, bytearray)) else text.encode("utf8")
    t, starts = decode_with_starts(text)
    if len(text) == 0:
        return [], [], t, starts
    toks, unk = _vocab(vocab)
    S = t + [1]
    for _, _, cps in toks:
        S += cps + [1]
    n = len(t)
    # per prefix flag: {length: {tuple(cps): id}}.  Duplicate lines: the reference's scanlines take the copy whose
    # suffix of S sorts last (a text position's suffix sorts behind every copy: its next code point is > 1) — the copy
    # followed by the greatest rest of the vocabulary stream
    after, q = [], n + 1
    for _, _, cps in toks:
        q += len(cps) + 1
        after.append(q)

    def later(i, j):  # S[after[i]:] > S[after[j]:]
        return greater(after[i], after[j])

    def greater(a, b):  # S[a:] > S[b:]
        while True:
            x, y = S[a:a + 64], S[b:b + 64]
            if x != y or not x:
                return x > y
            a += 64
            b += 64

    table, copies = ({}, {}), {}
    for i, (pf, bad, cps) in enumerate(toks):
        if not bad:
            d = table[pf].setdefault(len(cps), {})
            k = tuple(cps)
            copies.setdefault((pf, k), []).append(i)
            if k not in d or later(i, d[k]):
                d[k] = i

    def at_end(i, pf, k):
        # a match that ends the text: its suffix continues with 1 and the whole vocabulary stream — the nearest copy
        # behind it in suffix order, or in front of it when there is none
        c = copies[(pf, k)]
        if len(c) == 1:
            return i
        behind = [j for j in c if greater(after[j], n + 1)]
        if behind:
            return min(behind, key=lambda j: tuple(S[after[j]:after[j] + 4096]))
        return max(c, key=lambda j: tuple(S[after[j]:after[j] + 4096]))
    lens = tuple(sorted(table[0], reverse=True)), tuple(sorted(table[1], reverse=True))

    def wp(p):
        return p == 0 or is_spacing(t[p]) or is_spacing(t[p - 1])

    def best(p, prefix):
        for L in lens[prefix]:
            k = tuple(S[p:p + L])
            b = table[prefix][L].get(k)
            if b is not None:
                return (at_end(b, prefix, k) if p + L == n else b), L
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
            begin = spans[len(spans) - tsp][0] if tsp else p  # the first token the rollback drops
            del ids[len(ids) - tsp:]
            del spans[len(spans) - tsp:]
            tsp = 0
            p += 1
            while p < n and not wp(p):
                p += 1
            ids.append(unk)
            spans.append((begin, p))  # up to where the walk resumes
        while p < n and is_space(t[p]):
            p += 1
    return ids, spans, t, starts


def seq_len(lead):
    return 1 if lead < 0x80 else 2 if lead < 0xE0 else 3 if lead < 0xF0 else 4


def to_bytes(spans, text, starts):
    return [(starts[b], starts[e - 1] + seq_len(text[starts[e - 1]])) for b, e in spans]


def encode_with_offsets(text, vocab, unit="byte"):
    """-> (ids, [(begin, end)]) as Vocab.encode_with_offsets"""
    text = text if isinstance(text, (bytes, bytearray)) else text.encode("utf8")
    ids, spans, _, starts = encode_spans(text, vocab)
    return ids, (to_bytes(spans, text, starts) if unit == "byte" else spans)


def check_coverage(text, ids, spans_cp, t, starts):
    """The consequences the header states: increasing, disjoint, every non-blank code point in exactly one span, every
    uncovered byte part of a blank code point or dropped."""
    covered = [0] * len(t)
    prev = 0
    for b, e in spans_cp:
        assert prev <= b < e <= len(t), (prev, b, e)
        prev = e
        for q in range(b, e):
            covered[q] += 1
    for q, c in enumerate(t):
        assert covered[q] <= 1
        if not is_space(c):
            assert covered[q] == 1, (q, c)
    byte_spans = to_bytes(spans_cp, text, starts)
    inside = bytearray(len(text))
    for b, e in byte_spans:
        inside[b:e] = b"\x01" * (e - b)
    for q, s in enumerate(starts):
        if not inside[s]:
            assert is_space(t[q]), (q, t[q])
    return byte_spans


# ---- random small cases (shared by the CPU and GPU tests) ----
_CHARS = ["a", "b", "c", "é", "ж", "中", "文", "\U0001F600", "-", ",", " ", "\t", "▁", " "]


def random_case(rng):
    """(text bytes, vocab lines): hard or soft vocabs (a spacing char inside a multi-char token), with and without
    [UNK], invalid bytes, 2-4-byte characters, U+2581, CJK, leading and trailing blanks"""
    soft = rng.random() < 0.4
    letters = _CHARS[:8]
    vocab = set()
    for _ in range(rng.randint(1, 12)):
        k = rng.randint(1, 4)
        pool = _CHARS[:11] if soft else letters
        w = "".join(rng.choice(pool) for _ in range(k))
        if not soft and k > 1:
            w = "".join(c for c in w if not is_spacing(ord(c))) or "a"
        if rng.random() < 0.4:
            w = "##" + w
        vocab.add(w)
    for c in letters:  # most single letters, so that most words match
        if rng.random() < 0.7:
            vocab.add(c)
        if rng.random() < 0.5:
            vocab.add("##" + c)
    if rng.random() < 0.6:
        vocab.add("[UNK]")
    vocab = sorted(w for w in vocab if w.strip() and w != "##")
    rng.shuffle(vocab)
    parts = []
    if rng.random() < 0.3:
        parts.append(rng.choice([" ", "  ", "\t", "▁"]).encode())
    for _ in range(rng.randint(0, 30)):
        r = rng.random()
        if r < 0.05:
            parts.append(rng.choice([b"\xff", b"\xc3", b"\xe4\xb8", b"\x80", b"\xf0\x9f"]))
        else:
            parts.append(rng.choice(_CHARS).encode())
    if rng.random() < 0.3:
        parts.append(rng.choice([" ", "\n", "▁ "]).encode())
    return b"".join(parts), [w.encode() for w in vocab]
