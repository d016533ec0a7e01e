"""Pure-Python restatement of the vocabulary learner (include/wordpiece_amd.h, section "vocabulary learner"): the filters,
the substring counts, the top-down level pass, the iterations over the greedy split, the final list and the threshold
search, in plain dicts and lists.  Lengths are in code points.  A token is a pair (joined, text)."""


class TableError(ValueError):
    """what the device check of a table finds: a negative count, or a word that is not valid UTF-8"""


def filter_words(words, counts, reserved, max_token_chars, max_unique_chars):
    """-> (kept [(str, count)] in table order, stats).  Zero-byte words are skipped and count in n_words alone."""
    stats = dict(n_words=len(words), n_reserved=0, n_long=0, n_char_dropped=0)
    res = set(bytes(r) for r in reserved)
    kept = []
    for k, (w, c) in enumerate(zip(words, counts)):
        w = bytes(w)
        if c < 0:
            raise TableError("count of word %d is negative" % k)
        try:
            s = w.decode("utf8")
        except UnicodeDecodeError:
            raise TableError("word %d is not valid UTF-8" % k)
        if not w:
            continue
        if w in res or w.startswith(b"##"):
            stats["n_reserved"] += 1
        elif len(s) > max_token_chars:
            stats["n_long"] += 1
        else:
            kept.append((s, int(c)))
    if max_unique_chars > 0:
        occ = {}
        for s, c in kept:
            for ch in s:
                occ[ch] = occ.get(ch, 0) + c
        ranked = sorted(occ, key=lambda ch: (-occ[ch], ord(ch)))
        allowed = set(ranked[:max_unique_chars])
        left = [(s, c) for s, c in kept if all(ch in allowed for ch in s)]
        stats["n_char_dropped"] = len(kept) - len(left)
        kept = left
    return kept, stats


def greedy_split(s, kept):
    """the starts of the greedy longest-match split of s over the token set `kept` (single characters are always in)"""
    starts, p, n = [], 0, len(s)
    while p < n:
        starts.append(p)
        e = n
        while e > p + 1 and (p > 0, s[p:e]) not in kept:
            e -= 1
        p = e
    return starts


def one_threshold(words, chars, first, t, num_iterations, max_token_chars):
    """-> {token: score} of the last iteration: the kept tokens and every character, bare and joined"""
    kept = None
    for it in range(num_iterations):
        count = {}
        for s, c in words:
            n = len(s)
            starts = range(n) if it == 0 else greedy_split(s, kept)
            for b in starts:
                for e in range(b + 1, n + 1):
                    tok = (b > 0, s[b:e])
                    count[tok] = count.get(tok, 0) + c
        for tok in first:  # (a token none of whose occurrences is active counts 0)
            count.setdefault(tok, 0)
        kept = {}
        by_len = {}
        for tok in count:
            by_len.setdefault(len(tok[1]), []).append(tok)
        for length in range(max_token_chars, 0, -1):
            for tok in by_len.get(length, ()):
                c = count[tok]
                if c >= t:
                    kept[tok] = c
                    for k in range(1, length):
                        count[(tok[0], tok[1][:k])] -= c
        for ch in chars:
            kept.setdefault((False, ch), 1)
            kept.setdefault((True, ch), 1)
    return kept


def final_list(reserved, chars, kept, first):
    out = [(bytes(r).decode("utf8"), 0) for r in reserved]
    for ch in chars:
        out.append((ch, kept[(False, ch)]))
        out.append(("##" + ch, kept[(True, ch)]))
    rest = [tok for tok in kept if len(tok[1]) > 1]
    rest.sort(key=lambda tok: (-kept[tok], first[tok]))
    out += [(("##" if tok[0] else "") + tok[1], kept[tok]) for tok in rest]
    return out


def learn(words, counts, vocab_size, reserved=(b"[PAD]", b"[UNK]", b"[CLS]", b"[SEP]", b"[MASK]"), lower_thresh=10,
          upper_thresh=10_000_000, num_iterations=4, max_token_chars=50, max_unique_chars=1000, slack=None, slack_ratio=0.05):
    """words: bytes each; counts: ints -> dict(tokens=[str], scores=[int], thresh, stats)"""
    if slack is None:
        slack = int(slack_ratio * vocab_size)
    kept_words, stats = filter_words(words, counts, reserved, max_token_chars, max_unique_chars)
    chars = sorted(set(ch for s, _ in kept_words for ch in s))
    first, at = {}, 0  # first occurrence of every token in the order (word, s, e)
    for s, _ in kept_words:
        n = len(s)
        for b in range(n):
            for e in range(b + 1, n + 1):
                first.setdefault((b > 0, s[b:e]), at)
                at += 1
    stats.update(n_chars=len(chars), n_occurrences=at, n_tokens=len(first), n_steps=0, thresh=0)
    if not kept_words:
        return dict(tokens=[bytes(r).decode("utf8") for r in reserved], scores=[0] * len(reserved), thresh=0, stats=stats)
    lower, upper = lower_thresh, upper_thresh
    while True:
        t = (lower + upper) // 2
        stats["n_steps"] += 1
        kept = one_threshold(kept_words, chars, first, t, num_iterations, max_token_chars)
        out = final_list(reserved, chars, kept, first)
        size = len(out)
        if (size <= vocab_size and vocab_size - size <= slack) or lower >= upper or t <= 1:
            break
        if size > vocab_size:
            lower = t + 1
        else:
            upper = t - 1
    stats["thresh"] = t
    return dict(tokens=[x for x, _ in out], scores=[c for _, c in out], thresh=t, stats=stats)
