"""Generators and checks shared by the GPU tests of round 0 (test_gpu_blank_drop.py, test_gpu_round0_edges.py,
test_gpu_handle_state.py) and by the soak script: the sizes at which the default path changes its plan, read from the
headers; ASCII texts of an exact length with an exact number of blanks; the adversarial case kinds of the soak run, small
(make_case) and above 2^21 symbols (big_case); ids three ways (default, WP_OPT_SORT_BLANKS, WP_OPT_INDEXED_ROUND0) against
the oracle; the branch a case was built for, asserted from wp_stats.  Importing this module loads no library."""
import itertools
import os
import random
import re
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "wordpiece_amd", "csrc")

BLANKS = " \t\n\v\f\r"
SPACE_TOKEN = "▁"
LETTERS = "abcdefghijklmnopqrstuvwxyz"


def _define(header, name):
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(r"^#define\s+%s\s+(\d+)" % name, f.read(), re.M)
    assert m, (header, name)
    return int(m.group(1))


# ---- the constants the sizes below come from (csrc/): one place to edit if a header's expression changes
BLOCK = 256                                            # common.h, kBlock
RADIX_SMALL_N = 1 << 21                                # radix_sort.h, kRadixSmallN: above it the full-size tiles, the key
#                                                        builder's histogram (hist_in_keys) and with it the blank drop
TILE = BLOCK * _define("radix_sort.h", "WP_RADIX_ITEMS32")  # radix_sort.h, RadixCfg<Key0>::kTile (32-bit keys)
WINDOW_STORE_N = 1 << 22                               # linear_path.h, window_store = n >= 2^22
KEY_BITS = _define("code.h", "WP_KEY_BITS")            # code.h, kKeyBits
KEYS8_MIN_LEN = (KEY_BITS + 16) // 17                  # decode.h, kKeys8MinLen = (kKeyBits + kKeys8Items) / (kKeys8Items + 1)
MAX_CODE_LEN = 12                                      # code.h, kMaxCodeLen
BLANK_DROP_MIN_SHARE = 1.0 / 16                        # linear_path.h, kBlankDropMinShare
CODE_REUSE = 64                                        # linear_path.h, kCodeReuse
DEC_TILE = 16 << 10                                    # decode.h, kDecTile: the symbol histogram of a text of 64 tiles or
HIST_EVERY = 16                                        # more is taken from every 16th of them (decode_write_kernel)


def kept(text):
    """Suffixes the sort keeps: the non-blank positions of the text and the terminal one."""
    s = text.decode("utf-8")
    arr = np.frombuffer(s.encode("utf-32-le"), dtype=np.uint32)
    blank = np.isin(arr, np.array([ord(c) for c in BLANKS + SPACE_TOKEN], dtype=np.uint32))
    return int(arr.size - blank.sum()) + 1


def n_symbols(text):
    """n of an encode in the default layout: the code points of the text and the terminal symbol"""
    return len(text.decode("utf-8")) + 1


def letters_vocab(rng, n_words=3000):
    words = sorted({"".join(rng.choice(LETTERS) for _ in range(rng.randint(2, 12))) for _ in range(n_words)})
    vocab = ["[UNK]"] + list(LETTERS) + ["##" + c for c in LETTERS] + words + ["##" + w[:3] for w in words[:400]]
    return sorted(set(vocab)), words


def edge_vocab(seed):
    """letters_vocab, tokens far longer than a round-0 key (two and three words in one: they occur wherever the text glues
    words, so needed groups and the candidate list exist), tokens that begin with a blank, punctuation"""
    rng = random.Random(seed)
    vocab, words = letters_vocab(rng)
    long_tokens = [rng.choice(words) + rng.choice(words) + (rng.choice(words) if k % 2 else "") for k in range(300)]
    vocab += long_tokens + ["##" + w for w in long_tokens[:60]] + [" " + w for w in words[:20]] + [".", ",", "##."]
    return sorted(set(vocab)), words + long_tokens[:100]


def sized_text(seed, words, length, n_blank, blanks=BLANKS, end=None):
    """ASCII text of exactly `length` characters, exactly `n_blank` of them blanks (drawn from `blanks`): words of
    `words` one after another, blanks at word boundaries — one at as many boundaries as there are blanks for, the others
    glued; blanks beyond one per boundary go to random boundaries, the front and the back as longer runs.
    end: "blank" / "letter" forces the last character's kind."""
    rng = np.random.default_rng(seed)
    n_let = length - n_blank
    assert 0 <= n_blank <= length
    if n_let == 0:
        return bytes(rng.choice(np.frombuffer(blanks.encode(), np.uint8), size=length).tobytes())
    wl = np.array([len(w) for w in words])
    picks = []
    total = 0
    while total < n_let:
        idx = rng.integers(0, len(words), size=int(n_let / wl.mean()) + 64)
        picks.append(idx)
        total += int(wl[idx].sum())
    idx = np.concatenate(picks)
    ends = np.cumsum(wl[idx])
    letters = np.frombuffer("".join(words[i] for i in idx[:int(np.searchsorted(ends, n_let)) + 1]).encode(), np.uint8)[:n_let]
    inner = ends[ends < n_let]                      # slot i: behind letter i - 1 (slot 0: the front, n_let: the back)
    after = np.zeros(n_let + 1, dtype=np.int64)
    if n_blank <= inner.size:
        after[rng.choice(inner, size=n_blank, replace=False)] = 1
    else:
        after[inner] = 1
        slots = np.concatenate([inner, [0, n_let]])
        after += np.bincount(slots, weights=rng.multinomial(n_blank - inner.size, np.full(slots.size, 1.0 / slots.size)),
                             minlength=n_let + 1).astype(np.int64)
    if end == "letter" and after[n_let]:
        after[0] += after[n_let]
        after[n_let] = 0
    if end == "blank" and not after[n_let] and n_blank:
        j = int(np.argmax(after))
        after[j] -= 1
        after[n_let] += 1
    vals = np.full(2 * n_let + 1, 32, dtype=np.uint8)
    vals[1::2] = letters
    reps = np.ones(2 * n_let + 1, dtype=np.int64)
    reps[0::2] = after
    out = np.repeat(vals, reps)
    mask = out == 32
    out[mask] = rng.choice(np.frombuffer(blanks.encode(), np.uint8), size=int(mask.sum()))
    assert out.size == length and int(mask.sum()) == n_blank
    return out.tobytes()


def blank_fill(seed, text, lo, hi, blanks=BLANKS):
    """`text` with positions [lo, hi) overwritten by random blanks"""
    rng = np.random.default_rng(seed)
    out = np.frombuffer(text, np.uint8).copy()
    out[lo:hi] = rng.choice(np.frombuffer(blanks.encode(), np.uint8), size=hi - lo)
    return out.tobytes()


# ---- the symbol code the library builds (csrc/code.h), restated: a case that needs a codeword of a certain length checks
# here that its text yields one

def garsia_wachs(w):
    """optimal alphabetic code lengths for the weights w (code.h, garsia_wachs)"""
    n = len(w)
    if n == 1:
        return [1]
    INF = 1e300
    nodes = [(x, -1, -1, i) for i, x in enumerate(w)]
    seq = [-1] + list(range(n)) + [-1]

    def weight(i):
        return INF if i < 0 else nodes[i][0]

    while len(seq) > 3:
        i = 1
        while not weight(seq[i - 1]) <= weight(seq[i + 1]):
            i += 1
        nodes.append((weight(seq[i - 1]) + weight(seq[i]), seq[i - 1], seq[i], -1))
        new = len(nodes) - 1
        del seq[i - 1:i + 1]
        j = i - 2
        while weight(seq[j]) < nodes[new][0]:
            j -= 1
        seq.insert(j + 1, new)
    depth = [0] * n
    stack = [(seq[1], 0)]
    while stack:
        i, d = stack.pop()
        if nodes[i][3] >= 0:
            depth[nodes[i][3]] = d
        else:
            stack += [(nodes[i][1], d + 1), (nodes[i][2], d + 1)]
    return depth


def code_lengths(text, vocab):
    """{code point: codeword length} of the code build_symbol_code makes for an alphabet of at most 255 code points from
    the histogram of the whole text (the library samples large texts: lengths near a limit may differ by a bit), None
    where it falls back to a fixed width"""
    cps = np.frombuffer(text.decode("utf-8").encode("utf-32-le"), dtype=np.uint32)
    used = set(np.unique(cps).tolist()) | {1}
    for w in vocab:
        used |= {ord(c) for c in (w.decode("utf-8") if isinstance(w, bytes) else w)}
    order = sorted(used)
    uniq, cnt = np.unique(cps, return_counts=True)
    count = dict(zip(uniq.tolist(), cnt.tolist()))
    freq = [0.0] + [float(count.get(c, 0)) for c in order]  # (symbol 0: the padding behind the end)
    total = sum(freq)
    floor_div = 512.0
    while floor_div >= 32:
        lens = garsia_wachs([max(f, 1.0, total / floor_div) for f in freq])
        if max(lens) <= MAX_CODE_LEN:
            return dict(zip(order, lens[1:]))
        floor_div /= 2
    return None


# ---- child processes

_CHILD = '''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import %s as M
M.%s(*%r)
print("CHILD_OK")
'''
_child_no = itertools.count()


def run_in_child(tmp_path, module, func, args=(), env=None, timeout=900, check=True):
    """module.func(*args) in a fresh Python process with `env` added to the environment (WP_LIB: another build of the
    library; WP_NO_CONTEXT_POOL=1: every handle makes its own context, so no handle inherits the symbol code and the
    blank share an earlier handle of this process left in a parked one).  Returns the CompletedProcess; check: asserts
    that the function returned.  A child has its own time limit, and nothing follows a child that failed."""
    script = tmp_path / ("child_%d_%s.py" % (next(_child_no), func))
    script.write_text(_CHILD % (os.path.dirname(HERE), HERE, module, func, tuple(args)))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, **(env or {})))
    if check:
        assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return r


# ---- ids three ways

def three_ways(text, vocab, offsets=False):
    """ids (and byte offsets) of the default handle, WP_OPT_SORT_BLANKS=1 and WP_OPT_INDEXED_ROUND0=1; the default
    handle's statistics"""
    import wordpiece_amd as W
    res, st = [], None
    for opt in (None, W.WP_OPT_SORT_BLANKS, W.WP_OPT_INDEXED_ROUND0):
        gv = W.Vocab(vocab)
        if opt is not None:
            gv.set_option(opt, 1)
        if offsets:
            ids, offs = gv.encode_with_offsets(text)
            res.append((np.array(ids), np.array(offs)))
        else:
            res.append((gv.encode(text), None))
        if opt is None:
            st = gv.stats()
    return res, st


def check(text, vocab, exp=None, offsets=False):
    """the three handles agree (and equal exp); returns the default handle's statistics"""
    ((a, oa), (b, ob), (c, oc)), st = three_ways(text, vocab, offsets)
    if exp is not None:
        assert np.array_equal(a, exp), (len(text), vocab[:5])
    assert np.array_equal(a, b) and np.array_equal(a, c), (len(text), vocab[:5])
    if offsets:
        assert np.array_equal(oa, ob) and np.array_equal(oa, oc), (len(text), vocab[:5])
    return st


def assert_branch(st, text, keys_only=1, hist=None, drop=None, label=""):
    """The branch a case was built to reach, from wp_stats.  hist: the key builder took the sort's first histogram
    (hist_in_keys); drop: True — the sort left the blank-start suffixes out: round0_sorted is the kept count computed
    here, below n_total, and the passes ran over n + 3 * kept elements; False — it sorted every suffix."""
    n = n_symbols(text)
    assert st["n_total"] == n, (label, st["n_total"], n)
    assert st["round0_keys_only"] == keys_only, (label, st["round0_keys_only"])
    if hist is not None:
        assert st["hist_in_keys"] == hist, (label, st["hist_in_keys"])
    if drop:
        k = kept(text)
        assert st["round0_sorted"] == k < n, (label, st["round0_sorted"], k, n)
        assert st["radix_pass_elems"] == n + 3 * k, (label, st["radix_pass_elems"], n, k)
    elif drop is not None:
        assert st["round0_sorted"] == n, (label, st["round0_sorted"], n)


# ---- adversarial kinds (the soak run's), small

def make_case(rng, k):
    kind = k % 8
    if kind == 0:    # tiny alphabet, long repetitive text, long tokens (streams far beyond the 32-bit key)
        alpha, tok_max, text_len = "ab", 40, rng.randint(100, 20000)
    elif kind == 1:  # skewed alphabet: one very frequent symbol (1-2 bit code) and rare ones (12-bit codes)
        alpha, tok_max, text_len = "a" * 40 + "bcdefghijklmnopqrstuvwxyzABCDEFGH", 12, rng.randint(50, 8000)
    elif kind == 2:  # spacing chars inside tokens (soft), punctuation, CJK
        alpha, tok_max, text_len = "ab-, .c中文▁", 6, rng.randint(0, 3000)
    elif kind == 3:  # words with shared long prefixes
        alpha, tok_max, text_len = "abc ", 30, rng.randint(200, 30000)
    elif kind == 4:  # wide alphabet (> 255 symbols: u32 symbols, split code)
        alpha, tok_max, text_len = "".join(chr(c) for c in range(0x400, 0x400 + 300)) + " ab", 8, rng.randint(50, 5000)
    elif kind == 5:  # big case: full-size radix tiles and digit bytes (n > 2^21)
        alpha, tok_max, text_len = "etaoinshr dlu ", 20, rng.randint(2_200_000, 5_200_000)  # (> 2^22: LDS-window rank store, ranks inside its first pass)
    elif kind == 6:  # invalid UTF-8 sprinkled in
        alpha, tok_max, text_len = "ab c", 10, rng.randint(10, 2000)
    else:
        alpha, tok_max, text_len = "abcdefgh ij", 18, rng.randint(0, 6000)
    nt = rng.randint(1, 40)
    vocab = set()
    base = "".join(rng.choice(alpha.replace(" ", "")) for _ in range(tok_max)) if kind in (0, 3) else None
    while len(vocab) < nt:
        ln = rng.randint(1, tok_max)
        if base is not None and rng.random() < 0.6:
            w = base[:ln]  # prefixes of one long word: many long tokens with one key
        else:
            w = "".join(rng.choice(alpha) for _ in range(ln))
        if not w.strip():
            continue
        if rng.random() < 0.4:
            w = "##" + w
        vocab.add(w)
    vocab = sorted(vocab)
    rng.shuffle(vocab)
    if rng.random() < 0.4:
        vocab.append("[UNK]")
    if kind == 3 or kind == 0:
        words = [w.lstrip("#") for w in vocab if w != "[UNK]"] + [base]
        parts = []
        n = 0
        while n < text_len:
            w = rng.choice(words)
            cut = rng.randint(1, len(w))
            piece = w[:cut] + (rng.choice(words)[:rng.randint(0, 8)] if rng.random() < 0.5 else "")
            parts.append(piece)
            n += len(piece) + 1
        text = " ".join(parts)
    else:
        text = "".join(rng.choice(alpha) for _ in range(text_len))
    tb = text.encode("utf8")
    if kind == 6:
        bb = bytearray(tb)
        for _ in range(rng.randint(1, 6)):
            bb.insert(rng.randint(0, len(bb)), rng.choice([0xff, 0xc0, 0x80, 0xe2, 0xf0]))
        tb = bytes(bb)
    return tb, vocab


# ---- the same kinds above 2^21 symbols, with what the keys-only round 0 made interesting

BIG_KINDS = {0: ("ab", 40), 1: ("a" * 40 + "bcdefghijklmnopqrstuvwxyzABCDEFGH", 12), 3: ("abc ", 30),
             5: ("etaoinshr dlu ", 20), 7: ("abcdefgh ij", 18)}
BIG_FLAVOURS = ("plain", "blank_tokens", "blank_runs", "periodic", "crowded")


def big_case(seed, with_text=True):
    """Kind seed % 5 of (0, 1, 3, 5, 7) — two-letter alphabet with 40-symbol tokens, skewed alphabet, shared long prefixes,
    English-letter mix, mid alphabet — at 2.2 M to 5.2 M symbols, in flavour (seed // 5) % 5: plain; tokens that begin
    with or contain a blank; runs of 1 to 400 blanks; periodic words that put nearly every suffix on the candidate
    list; 20 k long tokens (the crowded candidate filter).  Returns (text, vocab, kind, flavour); with_text=False: the
    same vocabulary and no text."""
    rng = random.Random(1000 + seed)
    kind = sorted(BIG_KINDS)[seed % 5]
    flavour = BIG_FLAVOURS[(seed // 5) % 5]
    alpha, tok_max = BIG_KINDS[kind]
    text_len = rng.randint(2_200_000, 5_200_000)
    letters = "".join(sorted(set(alpha) - {" "}))
    nt = rng.randint(1, 40)
    vocab = set()
    base = "".join(rng.choice(letters) for _ in range(tok_max)) if kind in (0, 3) else None
    while len(vocab) < nt:
        ln = rng.randint(1, tok_max)
        w = base[:ln] if base is not None and rng.random() < 0.6 else "".join(rng.choice(alpha) for _ in range(ln))
        if not w.strip():
            continue
        vocab.add("##" + w if rng.random() < 0.4 else w)
    words = [w.lstrip("#") for w in sorted(vocab)] + ([base] if base else [])
    period = None
    if flavour == "blank_tokens":
        for w in words[:12]:
            vocab |= {" " + w, "\t" + w, w[:1] + " " + w[1:] + "x", "##" + w + " "}
    elif flavour == "periodic":
        period = "".join(rng.sample(letters, 2))
        vocab |= {period * k for k in (1, 2, 5, 9, 14, 20, 33, 40)} | {"##" + period * k for k in (1, 3, 7, 12, 21)}
        vocab |= {period[::-1] * k for k in (1, 4, 11, 25)} | {"##" + c for c in period} | set(period)
    elif flavour == "crowded":
        want = len(vocab) + 20000
        while len(vocab) < want:
            vocab.add("".join(rng.choices(letters, k=rng.randint(14, 24))))
    vocab = sorted(vocab)
    rng.shuffle(vocab)
    if rng.random() < 0.4:
        vocab.append("[UNK]")
    if not with_text:
        return None, vocab, kind, flavour
    parts, size = [], 0
    while size < text_len:
        if period and rng.random() < 0.85:
            piece = rng.choice((period * 40, period * 33 + rng.choice(letters), period[::-1] * 25))
        elif kind in (0, 3):
            w = rng.choice(words)
            piece = w[:rng.randint(1, len(w))] + (rng.choice(words)[:rng.randint(0, 8)] if rng.random() < 0.5 else "")
        else:
            piece = "".join(rng.choices(alpha, k=rng.randint(1, 4000)))
        if flavour == "blank_runs" and rng.random() < 0.3:
            sep = "".join(rng.choices(BLANKS, k=rng.randint(1, 400)))
        else:
            sep = " " if (kind in (0, 3) or period or flavour == "blank_runs") else ""
        parts.append(piece + sep)
        size += len(piece) + len(sep)
    return "".join(parts).encode("utf8"), vocab, kind, flavour
