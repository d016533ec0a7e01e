"""Constructed inputs for the refinement of the needed groups along the token trie — the stage between round 0 and the walk
(csrc/prune.h need_groups / needed_fill, csrc/trie.h, csrc/local_sort.h, linear_path.h::trie_round_finish, the group starts
of csrc/scanline.h) — a plain model of what the stage has to find, and what every case expects in wp_refine_stats and
wp_stats.  Shared by test_refine_cases.py (CPU) and test_gpu_refine_edges.py.  Importing this module loads no library.

The building block is a family: a stem of `depth` symbols whose first symbol (or first two, where a case needs more
families than one symbol allows) occurs nowhere else in text or vocabulary; tokens at chosen prefix lengths of the stem and
on branches off it; k words in the text that follow the stem for at least BASE = WP_KEY_BITS + 1 symbols — more than any
round-0 key holds, a codeword being at least one bit — and then leave it.  A suffix carries the key of a family's long tokens
exactly when it starts at one of the k members, so the family's needed group has k entries whatever code the text's
histogram yields (a head of two symbols needs both codewords inside the key: at most 2 x 12 bits, test_refine_cases.py
checks it with round0_cases.code_lengths).  The needed groups join the list in the order their atomics land, so populations
are chosen for edges that hold in every order; the two places where no population can do that say so below.

edge (issue bullet)                                         case(s)
G  one group of 2 / 64 / 65 / 256 / 257                     G_group_2 _64 _65 _256 _257 (G_group_2: the list is too short for
                                                            a large group, no classification runs)
   one group of kLsMaxGroup, stays in LDS                   G_group_max
   only groups of kLsMaxGroup: heads on window bounds       G_only_max
   only groups of kLsMaxGroup / 2                           G_only_half
   a window of 4095 entries                                 G_window_4095 (kLsMaxGroup - 1 among 4 of kLsMaxGroup: unless the
                                                            smaller group arrives last), G_window_16_rounds (only groups of
                                                            2040: two per window, 16 rounds of 256 in every order)
   2048+ groups of 2: a window full of heads                G_pairs_window
   63 / 64 / 65 and 4095 / 4096 / 4097 groups               G_groups_63 _64 _65 _4095 _4096 _4097 (sizes 2 and 3 mixed)
   a list of kLsT - 1 / kLsT / kLsT + 1 entries             G_list_T-1 G_list_T G_list_T+1
L  one group of kLsMaxGroup + 1 / of 5000                   L_group_max+1, L_group_5000
   three large groups, sizes that are / are no multiple of 64  L_three_large
   a window whose last owned group is large                 L_last_owned_large (6 small and 4 large groups: in all orders but
                                                            those that put every large group in front of every small one)
   a large group over more than two windows                 L_spans_windows
   only large groups                                        L_only_large
T  leaving at 1..20 and 8j - 1, 8j, 8j + 1 from a chain's start  T_leave_depths
   chains of 7 / 8 / 9 / 16 / 17 between branching nodes    T_chain_7 _8 _9 _16 _17
   full match that goes on / is followed by a blank         T_full_match_goes_on, T_full_match_blank
   the text ends 0..8 symbols into a chain                  T_text_end_0 .. T_text_end_8
   the stem's last token ends the vocabulary stream         T_last_token_in_stream
   a branching node with 1 / 2 / 3 / 40 children            T_children_1 _2 _3 _40
   the wanted child first / last / absent (3 ways)          T_child_first _last _absent_below _absent_between _absent_above
   a symbol no token holds behind a branching node          T_unknown_symbol
D  first branching node at depth 1..16                      D_branch_at_1 .. D_branch_at_16
   no member follows a long token beyond the key            D_no_member_follows
   first member and the others leave at different depths    D_first_member_differs
R  every prefix a token, depth 70 / every 7th               R_every_prefix_70, R_every_7th
   two long tokens part behind the key: +0 / +1 / +9        R_part_at_0 _1 _9
   ## token and prefix token of one word                    R_both_classes_one_node
   a ## family, members at in-word positions                R_inword_family
   tokens of kStepMaxLen - 1 / kStepMaxLen symbols          R_token_len_max-1, R_token_len_max
   a long token with 0 suffixes                             R_never_occurs
   ... with exactly one: match / sorts before / behind      R_once_match _before _behind
   every long token occurs once: nothing on the list        R_all_once
P  smallest / largest first symbol / both                   P_smallest, P_largest, P_both
N  trie_nodes + 1 = 2^8 - 1, 2^8, 2^8 + 1, 2^18 - 1 ...     N_nodes_255 _256 _257 _262143 _262144 _262145
Y  alphabets above 255 code points (32-bit symbols)         Y_group_65, Y_group_max+1, Y_three_large, Y_leave_depths,
                                                            Y_every_prefix_70, Y_pairs_300, Y_chain_9
F  seeded compositions                                      F_000 .. F_099

Wall time (measured): test_refine_cases.py 110 s for its 205 tests on the build container, single-threaded (the rest of
the CPU suite: 204 s); test_gpu_refine_edges.py: see that file."""
import functools
import os
import random
import re

import round0_cases as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "wordpiece_amd", "csrc")


def _constant(header, name):
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(r"^constexpr\s+\w+\s+%s\s*=\s*(\d+)(?:\s*<<\s*(\d+))?\s*;" % name, f.read(), re.M)
    assert m, (header, name)
    return int(m.group(1)) << int(m.group(2) or 0)


# ---- the constants the cases stand on: a changed constant moves the cases with it
LS_T = R._define("local_sort.h", "WP_LS_T")                # list entries per workgroup of the LDS sort
LS_MAXGROUP = R._define("local_sort.h", "WP_LS_MAXGROUP")  # larger groups take the global radix path
LS_BITS = _constant("local_sort.h", "kLsBits")             # bits per LSD pass of the window sort
LS_GROUP_BITS = _constant("local_sort.h", "kLsGroupBits")
LX_SPAN = _constant("local_sort.h", "kLxSpan")
WAVE = _constant("common.h", "kWave")
BLOCK = _constant("common.h", "kBlock")
KEY_BITS = R.KEY_BITS
STEP_MAX_LEN = _constant("scanline.h", "kStepMaxLen")
BASE = KEY_BITS + 1   # symbols every member shares with its stem: more than a key holds
assert LS_T == LS_MAXGROUP == 2048 and WAVE == 64 and LX_SPAN == 64 and KEY_BITS <= 32

BODY = "cdefgh"            # the symbols of the stems
LOW, HIGH = "ab", "xyz"    # leave symbols below / above every body symbol
HEADS1 = "ABCDEFGHIJKLMNOPQRSTUVWXYZ123456789"
# two-symbol heads: letters of Latin-1 and Latin Extended-A (no spacing chars), first and second symbol from disjoint pools
_LATIN = [chr(c) for c in range(0xC0, 0x180) if c not in (0xD7, 0xF7)]
HEADS2A, HEADS2B = _LATIN[:64], _LATIN[64:130]
# wide alphabets: Greek and Cyrillic letters (none is a spacing char); with _LATIN more than 255 code points
_GREEK = [chr(c) for c in range(0x391, 0x3CA) if c != 0x3A2]
_CYRILLIC = [chr(c) for c in range(0x400, 0x480)]
# (in this order no two neighbours of the filler word make a two-symbol head of _wide_heads: Greek first, Cyrillic second)
WIDE_FILL = "".join(_CYRILLIC + _GREEK + _LATIN)
assert len(set(WIDE_FILL)) > 300 and len(HEADS2A) * len(HEADS2B) >= 4160


def bit_length(v):
    return int(v).bit_length()


def stem_of(head, depth, salt=0):
    """head + body symbols, fixed by (head, salt): no two stems share a first symbol, so their content is free"""
    rng = random.Random("%s/%d" % (head, salt))
    return head + "".join(rng.choice(BODY) for _ in range(depth - len(head)))


class Family:
    """stem, tokens and member words of one family.  at: prefix lengths of the stem that are tokens; branches: (d, tail)
    -> token stem[:d] + tail; leaves: (d, tail) -> word stem[:d] + tail, dealt to the k members in turn; cls: "" / "##" /
    "both" — the class of the stem's tokens; inword: every member word gets this symbol in front (in-word members)."""

    def __init__(self, head, depth=BASE + 4, at=None, branches=(), leaves=None, k=2, cls="", inword="", stem=None):
        self.head, self.k = head, k
        self.stem = stem if stem is not None else stem_of(head, depth)
        depth = len(self.stem)
        words = [self.stem[:L] for L in (at if at is not None else [depth])] + [self.stem[:d] + t for d, t in branches]
        self.words = words
        self.tokens = []
        for w in words:
            if cls in ("", "both"):
                self.tokens.append(w)
            if cls in ("##", "both"):
                self.tokens.append("##" + w)
        if leaves is None:
            leaves = [(depth, HIGH[0]), (max(BASE, depth - 2), HIGH[1]), (max(BASE, depth - 3), LOW[0]), (depth, "")]
        self.leaves = list(leaves)
        self.members = []
        for i in range(k):
            d, t = self.leaves[i % len(self.leaves)]
            assert d >= BASE or k == 1, (head, d)
            self.members.append(inword + self.stem[:d] + t)
        self.listed = k >= 2 and any(len(w) >= BASE and w[:BASE] == self.stem[:BASE] for w in words)


class Case:
    def __init__(self, name, families, seed=0, extra_tokens=(), last_word=None, wide=False, last_token=None, singles=True,
                 text_only_symbols=""):
        self.name, self.families = name, families
        rng = random.Random(seed)
        words = [w for f in families for w in f.members]
        rng.shuffle(words)
        if wide:
            words.insert(len(words) // 2, WIDE_FILL)
        if last_word is not None:
            words.append(last_word)
        self.text = " ".join(words).encode("utf-8")
        toks = [t for f in families for t in f.tokens] + list(extra_tokens)
        used = sorted(set("".join(words)) - set(" ") - set(text_only_symbols))
        vocab = ["[UNK]"] + ([c for c in used] + ["##" + c for c in used] if singles else [])
        vocab += sorted(set(toks) - set(vocab))
        if last_token is not None:  # (the vocabulary stream follows the order of the lines)
            vocab.remove(last_token)
            vocab.append(last_token)
        assert len(set(vocab)) == len(vocab)
        self.vocab = vocab
        heads = [f.head for f in families]
        assert len(set(heads)) == len(heads) and len({h[0] for h in heads} & set("".join(f.stem[len(f.head):] for f in families))) == 0


def trie_nodes(vocab):
    """nodes of the trie of the eligible tokens' words (csrc/vocab.h, build_token_trie): the root and one node per
    distinct non-empty prefix — counted over the sorted words as len(w) - lcp(w, predecessor)"""
    words = sorted({w[2:] if w.startswith("##") else w for w in vocab if w != "[UNK]"})
    n, prev = 1, ""
    for w in words:
        l = 0
        while l < len(prev) and l < len(w) and prev[l] == w[l]:
            l += 1
        n += len(w) - l
        prev = w
    return n


def expected_stats(case):
    """what the default handle reports for the case, from the construction: (wp_refine_stats fields, wp_stats fields)"""
    sizes = [f.k for f in case.families if f.listed]
    n_entries = sum(sizes)
    alphabet = len(set(case.text.decode("utf-8")) | set("".join(w[2:] if w.startswith("##") else w for w in case.vocab)) | {"\x01"})
    nodes = trie_nodes(case.vocab)
    one_byte = alphabet <= 255
    n_total = len(case.text.decode("utf-8")) + 1
    # (the large groups are classified when the list's room — the whole text while the handle has no memory of an earlier
    # encode and the text is short — could hold one: linear_path.h, classify_groups(list_cap))
    list_cap = min(n_total, n_total // 8 + n_total // 8 // 4 + 65536)
    classified = list_cap > LS_MAXGROUP
    large = [s for s in sizes if s > LS_MAXGROUP] if classified else []
    refine = dict(n_groups=len(sizes), n_entries=n_entries, n_large_groups=len(large), n_large_entries=sum(large),
                  trie_nodes=nodes, sort_bits=bit_length(nodes + 1), key_lookup=1, symbol_bytes=1 if one_byte else 4)
    stats = dict(trie_refine=1, round0_keys_only=1 if one_byte else 0, needed_after_round0=n_entries,
                 rounds=2 if n_entries else 1, n_total=n_total)
    return refine, stats


# ---- the model ------------------------------------------------------------------------------------------------------------

def longest_matches(text, vocab):
    """For every code point position of the text: (id of the longest prefix-class token that is a prefix of the text there,
    id of the longest ##-class token), -1 where there is none.  A dict trie; special tokens ([...]) match nothing."""
    t = text.decode("utf-8") if isinstance(text, (bytes, bytearray)) else text
    root = {}
    for i, w in enumerate(vocab):
        w = w.decode("utf-8") if isinstance(w, (bytes, bytearray)) else w
        cls = 0
        if w.startswith("##"):
            cls, w = 1, w[2:]
        elif len(w) > 2 and w[0] == "[" and w[-1] == "]":
            continue
        node = root
        for c in w:
            node = node.setdefault(c, {})
        node.setdefault(None, [-1, -1])[cls] = i
    out_p, out_s = [-1] * len(t), [-1] * len(t)
    n = len(t)
    for p in range(n):
        node, q, bp, bs = root, p, -1, -1
        while q < n:
            node = node.get(t[q])
            if node is None:
                break
            q += 1
            end = node.get(None)
            if end is not None:
                if end[0] >= 0:
                    bp = end[0]
                if end[1] >= 0:
                    bs = end[1]
        out_p[p], out_s[p] = bp, bs
    return out_p, out_s


def group_populations(text, vocab):
    """{first BASE symbols of a token of at least BASE symbols: text positions that start with them}: the direct count the
    expected list sizes are checked against"""
    t = text.decode("utf-8")
    out = {}
    for w in vocab:
        w = w[2:] if w.startswith("##") else w
        if len(w) >= BASE:
            out.setdefault(w[:BASE], [])
    first = {k[0] for k in out}
    for p, ch in enumerate(t):
        if ch in first:
            pos = out.get(t[p:p + BASE])
            if pos is not None:
                pos.append(p)
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------

CASES = {}


def case(name):
    def deco(f):
        assert name not in CASES, name
        CASES[name] = f
        return f
    return deco


def _heads(n):
    """n distinct heads: single symbols while they last, else two symbols from disjoint pools"""
    if n <= len(HEADS1):
        return list(HEADS1[:n])
    assert n <= len(HEADS2A) * len(HEADS2B)
    return [HEADS2A[i % len(HEADS2A)] + HEADS2B[i // len(HEADS2A)] for i in range(n)]


def _wide_heads(n):
    pool = _GREEK + _CYRILLIC
    if n <= len(pool):
        return pool[:n]
    return [_GREEK[i % len(_GREEK)] + _CYRILLIC[i // len(_GREEK)] for i in range(n)]


def _sized(name, sizes, wide=False, **kw):
    """one family per size; tokens at BASE + 1 and at the stem's end, members leaving at four depths"""
    heads = (_wide_heads if wide else _heads)(len(sizes))

    @case(name)
    def _():
        return Case(name, [Family(h, at=[BASE + 1, BASE + 4], k=k, **kw) for h, k in zip(heads, sizes)], wide=wide)


for _k in (2, 64, 65, 256, 257):
    _sized("G_group_%d" % _k, [_k])
_sized("G_group_max", [LS_MAXGROUP])
_sized("G_only_max", [LS_MAXGROUP] * 5)
_sized("G_only_half", [LS_MAXGROUP // 2] * 6)
_sized("G_window_4095", [LS_MAXGROUP - 1] + [LS_MAXGROUP] * 4)
_sized("G_window_16_rounds", [LS_MAXGROUP - 8] * 5)
_sized("G_pairs_window", [2] * (LS_T + 60))
for _g in (63, 64, 65, 4095, 4096, 4097):
    _sized("G_groups_%d" % _g, [2 + (i * 7 % 3 == 0) for i in range(_g)])
for _d in (-1, 0, 1):
    _sized("G_list_T%s" % ("%+d" % _d if _d else ""), [1000, 600, LS_T - 1600 + _d])

_sized("L_group_max+1", [LS_MAXGROUP + 1])
_sized("L_group_5000", [5000])
_sized("L_three_large", [LS_MAXGROUP + 1, 33 * LX_SPAN, 3000, 5])
_sized("L_last_owned_large", [100] * 6 + [2500] * 4)
_sized("L_spans_windows", [3 * LS_T + 100, 7, 300])
_sized("L_only_large", [LS_MAXGROUP + 1, 2600, 2 * LS_T])

CHAIN0 = BASE + 1   # depth of the node behind the child step off the branching node at depth BASE: a chain starts here


def _every(stem):
    """every prefix of the stem from BASE symbols on is a token: a member's longest match is the depth at which it leaves"""
    return list(range(BASE, len(stem) + 1))


def _branch(stem, d, n=3):
    """a tail that parts from the stem at depth d: a body symbol other than the stem's, then n more"""
    other = BODY[(BODY.index(stem[d]) + 1) % len(BODY)] if d < len(stem) and stem[d] in BODY else BODY[0]
    return other + BODY[0] * n


@case("T_leave_depths")
def _():
    offs = list(range(1, 21)) + [8 * j + e for j in range(3, 10) for e in (-1, 0, 1)]
    stem = stem_of("T", CHAIN0 + max(offs) + 3)
    return Case("T_leave_depths", [Family("T", stem=stem, at=_every(stem), branches=[(BASE, _branch(stem, BASE))],
                                          leaves=[(CHAIN0 + o, HIGH[o % 3]) for o in offs] + [(CHAIN0, LOW[0])], k=2 * len(offs) + 3)])


def _chain_case(name, L, wide=False):
    @case(name)
    def _():
        head = _wide_heads(1)[0] if wide else "T"
        stem = stem_of(head, CHAIN0 + L + 12)
        b2 = CHAIN0 + L  # second branching node: a chain of L nodes lies between the two
        leaves = [(d, t) for d in (CHAIN0, CHAIN0 + 1, b2 - 1, b2, b2 + 1, len(stem)) for t in (LOW[1], HIGH[2])]
        leaves += [(BASE, _branch(stem, BASE)), (b2, _branch(stem, b2)), (b2, _branch(stem, b2)[:2] + HIGH[0]), (len(stem), "")]
        return Case(name, [Family(head, stem=stem, at=_every(stem), branches=[(BASE, _branch(stem, BASE)), (b2, _branch(stem, b2))],
                                  leaves=leaves, k=2 * len(leaves))], wide=wide)


for _L in (7, 8, 9, 16, 17):
    _chain_case("T_chain_%d" % _L, _L)


@case("T_full_match_goes_on")
def _():
    return Case("T_full_match_goes_on", [Family("T", at=[BASE, BASE + 9], leaves=[(BASE + 9, "xc"), (BASE + 9, "c" * 9), (BASE + 2, "y")], k=7)])


@case("T_full_match_blank")
def _():
    return Case("T_full_match_blank", [Family("T", at=[BASE, BASE + 9], leaves=[(BASE + 9, ""), (BASE, ""), (BASE + 9, "")], k=8)])


def _text_end(o):
    @case("T_text_end_%d" % o)
    def _():
        stem = stem_of("T", CHAIN0 + 20)
        f = Family("T", stem=stem, at=_every(stem), branches=[(BASE, _branch(stem, BASE))], k=5)
        f.k += 1  # (the last word of the text is a member too)
        return Case("T_text_end_%d" % o, [f, Family("U", k=3)], last_word=stem[:CHAIN0 + o])


for _o in range(9):
    _text_end(_o)


@case("T_last_token_in_stream")
def _():
    f = Family("T", at=[BASE, BASE + 11], k=6)
    return Case("T_last_token_in_stream", [Family("A", k=3), f], last_token=f.stem)


def _children(name, nch, wanted=None):
    """a branching node at depth BASE with nch children; members into the first, a middle and the last child, and past the
    node with symbols below, between and above the children (wanted: only that one way, twice two members)"""
    @case(name)
    def _():
        stem = stem_of("T", BASE + 6)
        pool = (BODY if nch <= 3 else "".join(HEADS2A[:nch]))
        kids = sorted(set(pool) - {stem[BASE]})[:nch - 1] if nch > 1 else []
        kids = sorted(kids + [stem[BASE]])
        if nch == 3:
            kids = ["d", "f", "h"]
            stem = stem[:BASE] + "f" + stem[BASE + 1:]
        ways = {"first": kids[0] + "cc", "last": kids[-1] + "cc", "absent_below": LOW[0] + "c", "absent_above": HIGH[2] + "c",
                "absent_between": ("e" if nch == 3 else LOW[1]) + "c", "middle": kids[len(kids) // 2] + "cc"}
        tails = [ways[wanted], ways[wanted][:1]] if wanted else sorted(ways.values())
        branches = [(BASE, c + "cc") for c in kids if c != stem[BASE]]
        return Case(name, [Family("T", stem=stem, at=[BASE, len(stem)], branches=branches,
                                  leaves=[(BASE, t) for t in tails] + [(BASE + 3, HIGH[0])], k=2 * len(tails) + 2)])


for _n in (1, 2, 3, 40):
    _children("T_children_%d" % _n, _n)
for _w in ("first", "last", "absent_below", "absent_between", "absent_above"):
    _children("T_child_%s" % _w, 3, _w)


@case("T_unknown_symbol")
def _():
    stem = stem_of("T", BASE + 6)
    return Case("T_unknown_symbol", [Family("T", stem=stem, at=[len(stem)], branches=[(BASE, _branch(stem, BASE))],
                                            leaves=[(BASE, "q"), (BASE, "qc"), (BASE + 6, "q"), (BASE + 2, "x")], k=8)], text_only_symbols="q")


def _d_branch(b):
    @case("D_branch_at_%d" % b)
    def _():
        stem = stem_of("D", BASE + 8)
        return Case("D_branch_at_%d" % b, [Family("D", stem=stem, at=_every(stem), branches=[(b, _branch(stem, b, 30)), (b, _branch(stem, b, 2))],
                                                  k=9), Family("E", k=2)])


for _b in range(1, 17):
    _d_branch(_b)


@case("D_no_member_follows")
def _():
    stem = stem_of("D", BASE + 8)
    return Case("D_no_member_follows", [Family("D", stem=stem, at=[], branches=[(BASE, _branch(stem, BASE, 4))],
                                               leaves=[(BASE, "x"), (BASE + 5, "y"), (BASE, "")], k=6)])


@case("D_first_member_differs")
def _():
    return Case("D_first_member_differs", [Family("D", depth=BASE + 20, at=[BASE + 2, BASE + 20],
                                                  leaves=[(BASE, "a")] + [(BASE + 20, "x")] * 10, k=33)])


@case("R_every_prefix_70")
def _():
    return Case("R_every_prefix_70", [Family("R", depth=70, at=list(range(1, 71)), leaves=[(d, "x") for d in range(BASE, 71)], k=3 * (71 - BASE))])


@case("R_every_7th")
def _():
    return Case("R_every_7th", [Family("R", depth=70, at=list(range(7, 71, 7)), leaves=[(d, "x") for d in range(BASE, 71)], k=2 * (71 - BASE))])


def _part(e):
    @case("R_part_at_%d" % e)
    def _():
        stem = stem_of("R", BASE + e + 6)
        br = (BASE + e, _branch(stem, BASE + e, 5))
        return Case("R_part_at_%d" % e, [Family("R", stem=stem, at=[len(stem)], branches=[br],
                                                leaves=[(len(stem), "x"), br, (BASE + e, "x"), (br[0], br[1][:2]), (BASE, "a")], k=15)])


for _e in (0, 1, 9):
    _part(_e)


@case("R_both_classes_one_node")
def _():
    f = Family("R", at=[BASE, BASE + 4], cls="both", k=6)
    g = Family("S", at=[BASE, BASE + 4], cls="both", k=6, inword="c")
    return Case("R_both_classes_one_node", [f, g])


@case("R_inword_family")
def _():
    return Case("R_inword_family", [Family("R", at=[BASE - 3, BASE, BASE + 4], cls="##", k=40, inword="dc")])


def _token_len(name, L):
    @case(name)
    def _():
        return Case(name, [Family("R", depth=L, at=[BASE, L // 2, L], leaves=[(L, ""), (L, "x"), (L - 1, "x"), (BASE, "y")], k=4)])


_token_len("R_token_len_max-1", STEP_MAX_LEN - 1)
_token_len("R_token_len_max", STEP_MAX_LEN)


@case("R_never_occurs")
def _():
    return Case("R_never_occurs", [Family("R", k=5)], extra_tokens=[stem_of("N", BASE + 7), "##" + stem_of("O", BASE + 3)])


def _once(way):
    @case("R_once_%s" % way)
    def _():
        leave = {"match": (BASE + 4, "x"), "before": (BASE + 1, "a"), "behind": (BASE + 1, "z")}[way]
        return Case("R_once_%s" % way, [Family("R", leaves=[leave], k=1), Family("S", k=4)])


for _w in ("match", "before", "behind"):
    _once(_w)


@case("R_all_once")
def _():
    return Case("R_all_once", [Family(h, leaves=[lv], k=1) for h, lv in zip("RST", [(BASE + 4, ""), (BASE, "a"), (BASE + 2, "z")])])


@case("P_smallest")
def _():
    return Case("P_smallest", [Family("0", k=7), Family("M", k=3)])


@case("P_largest")
def _():
    return Case("P_largest", [Family("ſ", k=7), Family("M", k=3)])


@case("P_both")
def _():
    return Case("P_both", [Family("0", k=5), Family("ſ", k=6), Family("M", k=3)])


def _nodes(total):
    """trie_nodes + 1 == total: two families (a small and a large group) and filler tokens that never occur"""
    @case("N_nodes_%d" % total)
    def _():
        fams = [Family("A", k=3), Family("B", k=LS_MAXGROUP + 1)]
        base = Case("", fams)
        want = total - 1 - trie_nodes(base.vocab)
        filler, i = [], 0
        while want > 0:   # each filler: its own two-symbol head (the first symbol is new for the first 64), body symbols
            shared = 1 if i >= 64 else 0
            L = min(want + shared, 512)
            if 0 < want - (L - shared) < 3:
                L -= 3
            filler.append(stem_of(HEADS2A[i % 64] + HEADS2B[i // 64], L))
            want -= L - shared
            i += 1
        c = Case("N_nodes_%d" % total, fams, extra_tokens=filler)
        assert trie_nodes(c.vocab) + 1 == total, (trie_nodes(c.vocab), total)
        return c


for _t in (255, 256, 257, (1 << 18) - 1, 1 << 18, (1 << 18) + 1):
    _nodes(_t)

# ---- wide alphabets: the same shapes on 32-bit symbols
_sized("Y_group_65", [65], wide=True)
_sized("Y_group_max+1", [LS_MAXGROUP + 1], wide=True)
_sized("Y_three_large", [LS_MAXGROUP + 1, 33 * LX_SPAN, 2500, 5], wide=True)
_sized("Y_pairs_300", [2 + (i % 5 == 0) for i in range(300)], wide=True)
_chain_case("Y_chain_9", 9, wide=True)


@case("Y_leave_depths")
def _():
    h = _wide_heads(1)[0]
    offs = list(range(1, 21)) + [8 * j + e for j in range(3, 6) for e in (-1, 0, 1)]
    stem = stem_of(h, CHAIN0 + max(offs) + 3)
    return Case("Y_leave_depths", [Family(h, stem=stem, at=_every(stem), branches=[(BASE, _branch(stem, BASE))],
                                          leaves=[(CHAIN0 + o, HIGH[o % 3]) for o in offs], k=2 * len(offs))], wide=True)


@case("Y_every_prefix_70")
def _():
    h = _wide_heads(2)[1]
    return Case("Y_every_prefix_70", [Family(h, depth=70, at=list(range(1, 71)), leaves=[(d, "x") for d in range(BASE, 71)], k=2 * (71 - BASE))], wide=True)


# ---- group F: seeded compositions
F_SEEDS = 100
_F_SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, LS_MAXGROUP // 2, LS_MAXGROUP - 1, LS_MAXGROUP, LS_MAXGROUP + 1, 2 * LS_T + 70]


def _composed(seed):
    rng = random.Random(7000 + seed)
    wide = seed % 10 == 9
    nf = rng.randint(2, 6)
    heads = (_wide_heads if wide else _heads)(40)
    rng.shuffle(heads)
    fams, budget = [], 3000
    for h in heads[:nf]:
        k = rng.choice([s for s in _F_SIZES if s <= max(budget, 3)])
        budget -= k
        depth = BASE + rng.choice([1, 4, 9, 17, 37])
        stem = stem_of(h, depth, seed)
        shape = rng.randrange(4)
        at = {0: [depth], 1: list(range(1, depth + 1)), 2: list(range(7, depth + 1, 7)) + [depth], 3: [BASE, depth]}[shape]
        nb = rng.randint(0, 3)
        branches = [(d, _branch(stem, d, rng.randint(0, 9))) for d in sorted({rng.randint(1, depth - 1) for _ in range(nb)})]
        leaves = [(rng.randint(BASE, depth), rng.choice(["", "x", "a", "zc", "y"])) for _ in range(rng.randint(1, 12))]
        leaves += [(d, t[:rng.randint(1, len(t))]) for d, t in branches if d >= BASE]
        cls = rng.choice(["", "", "##", "both"])
        fams.append(Family(h, stem=stem, at=at, branches=branches, leaves=leaves, k=k, cls=cls, inword="c" if cls == "##" else ""))
    return Case("F_%03d" % seed, fams, seed=seed, wide=wide)


for _s in range(F_SEEDS):
    CASES["F_%03d" % _s] = functools.partial(_composed, _s)

GROUPS = ("G", "L", "T", "D", "R", "P", "N", "Y", "F")


def names(groups="GLTDRPNY"):
    return [n for n in CASES if n[0] in groups]


@functools.lru_cache(maxsize=8)
def build(name):
    c = CASES[name]()
    c.name = name
    return c


def between_text(case_):
    """a text of another population for the same vocabulary, encoded between two encodes of a case: a large group for a case
    of group G, groups of three for the others"""
    if case_.name[0] == "G":
        f = case_.families[0]
        return " ".join([f.members[0], f.members[-1]] * (LS_MAXGROUP // 2 + 3)).encode("utf-8")
    return " ".join(w for f in case_.families for w in (f.members * 3)[:3]).encode("utf-8")


# one case each of G (the 4095-entry window), L (three large groups), T (the text ends in a chain) and P, embedded at size
EMBEDDED = ["G_window_4095", "L_three_large", "T_text_end_3", "P_both"]
# no WP_OPT_VOCAB_IN_S run: the doubling rounds over a vocabulary of 2^18 symbols in S take long (and N is not asked for)
VOCAB_IN_S_GROUPS = "GLRP"
