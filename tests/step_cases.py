"""Constructed inputs for the stage between the sort and the walk — the scanlines of csrc/scanline.h, virtual_marks_kernel
of csrc/prune.h and linear_path.h::scanlines / side_tables / fill_tables, which turn "which token is the longest match at this suffix" into
the step tables the walk reads — a plain model of what the stage has to find (refine_cases.longest_matches, unchanged), and
what every case claims.  Shared by test_step_cases.py (CPU) and test_gpu_step_edges.py.  Importing this module loads no
library.

T = kBlock * kSlItems = 4096 slots per tile, G = kSlGroup * T slots per group of tiles.

Family S (slot space: S = text . 1 . vocab, WP_OPT_VOCAB_IN_S or U+0000 in the text).  The focus token is the one-symbol
word "m".  In S every vocabulary line ends with the separator U+0001, which sorts below every text symbol but U+0000: the
suffix of the line "m" is the first suffix that starts with "m", behind it come the f text occurrences "m " (the forward
run), in front of it the b occurrences "m<U+0000>" (the backward run), and the mark's slot is the number of symbols of S
below "m" plus b.  Padding words "a" / "aa" in front and words of "z" behind move the slot and the length of S to any value;
_fit does the arithmetic and test_step_cases.py proves the outcome from the oracle's who / SA / lcp.

edge (issue bullet)                                          case(s)
S  forward run of 0 1 62 63 64 65 127 128 129                S_fwd_<f>
   backward run of the same                                  S_bwd_<b>
   local slot 0 1 63 64 T-2 T-1                              S_local_<l>
   last tile of 1 / T-1 slots                                S_last_tile_1, S_last_tile_T-1
   reach ends at the tile's last slot / at the boundary /    S_end_last_slot, S_end_boundary, S_end_next_1, S_end_n
   one slot on / at n
   forward over 1 2 63 64 65 whole tiles, stop in the        S_tiles_1_own S_tiles_1_next S_tiles_2_own S_tiles_2_next
   mark's own group / the next / the one behind it           S_tiles_63 S_tiles_64 S_tiles_65 S_tiles_65_two_groups
   backward over 1 and 2 tiles, into the previous group      S_back_tiles_1, S_back_tiles_2, S_back_group
   a stop more than 64 groups behind the mark's group        S_far_group (n = 34.4 M; ids only; its own GPU test)
   two marks of one class: nested, same end, disjoint        S_two_nested, S_two_same_end, S_two_disjoint
   both classes on one string                                S_both_classes
   duplicate lines (full depth is forced)                    S_dup_same_class, S_dup_both_classes
   0 1 63 64 65 eligible tokens                              S_tokens_<M>
K  M = 63 64 65 4096 4097 (the 64-ary search) and            K_marks_<M>  (both classes interleaved; the covering token "b"
   8191 8192 8193 16385 (the carry of mark_cover_kernel)     is mark 0, the slots of "bz" lie behind the last mark)
   covering mark k marks in front, k = 1 63 64 65 129,       K_cover_<k>_same, K_cover_<k>_other
   the k marks in the same / the other class
   k tokens in a row that never occur, k = 1 64 65           K_empty_<k>
   a chain of nested prefixes of 1..7 symbols, both classes  K_chain
   a range that starts at the first non-blank slot / ends    K_first_slot_token, K_first_slot_prefix,
   at n; the last word the token / only its prefix matches   K_last_slot_token, K_last_slot_prefix
   n_total = 2^18 - 1, 2^18, 2^18 + 1, 2^19 + 1              K_n_262143 K_n_262144 K_n_262145 K_n_524289
   bit_length(4 P) on both sides of kStepBucketBits, a text  K_shift_all_16383, K_shift_all_16384 (one word of more
   above 2^19 symbols: bucket_shift_all != bucket_shift      than 2048 positions, a stretch of ordinary words)
   a vocabulary of 2^20 - 1 / 2^20 lines: packed 1 / 0       K_pack_1048575, K_pack_1048576
   a needed group beside a K vocabulary                      K_with_family
   32-bit symbols                                            K_wide_cover_65, K_wide_chain, K_wide_marks_8193
F  seeded compositions over 3-4 symbols, 1-3 tiles           F_000 .. F_047 (both layouts, no claims)

Not covered, and why.  The gb -= kWave loop of sl_reach_global_kernel in the BACKWARD direction past 64 groups: it needs
17.1 M occurrences of "m<U+0000>" and would double the largest input.  For the two vocabularies of 2^20 - 1 and 2^20 lines
(K_pack_*) the oracle and the model take 6 s and 3 s on the build host, so both stay the reference; on the GPU they run the
default handle, the step views, the debug views and the fast path, not the option matrix and not the second population
(every handle parses the million lines again).

n_steps of a K case: two starts per needed group join the step list, and the groups depend on the symbol code, which a
handle may inherit from an earlier text with the same alphabet (a parked context).  The GPU file therefore takes the number of
groups of a first encode from wp_refine_stats (at least what the construction brings) and asserts the construction's exact
number only behind the text of another alphabet, where the handle holds the case's own code — the code under which
test_step_cases.py proves that no other token outgrows a key.  Wide-symbol cases (low bits verbatim in the key) never assert it.

Wall time (measured on the build container, single-threaded): test_step_cases.py 45 s for its 142 tests, 25 s of it the two
vocabularies of 2^20 lines (the rest of the CPU suite: 250 s); test_gpu_step_edges.py: 61 s on an MI355X, 6.2 % on top of the
rest of the -m gpu suite (the figures and the two mutation counts stand in that file's docstring)."""
import functools
import os
import random

import refine_cases as RC
import round0_cases as R

longest_matches = RC.longest_matches   # the model: longest prefix-class / ##-class token at every text position
bit_length = RC.bit_length

# ---- the constants the cases stand on
SL_ITEMS = RC._constant("scanline.h", "kSlItems")
SL_GROUP = RC._constant("scanline.h", "kSlGroup")
COVER_THREADS = RC._constant("scanline.h", "kCoverThreads")
COVER_ITEMS = RC._constant("scanline.h", "kCoverItems")
STEPS_PER_MARK = RC._constant("scanline.h", "kStepsPerMark")
STEP_BUCKET_BITS = R._define("scanline.h", "WP_STEP_BUCKET_BITS")
STEP_BUCKET_BITS_MAX = R._define("scanline.h", "WP_STEP_BUCKET_BITS_MAX")
STEP_ID_BITS = RC._constant("scanline.h", "kStepIdBits")
STEP_MAX_LEN = RC.STEP_MAX_LEN
BLOCK, WAVE, KEY_BITS = RC.BLOCK, RC.WAVE, RC.KEY_BITS
T = BLOCK * SL_ITEMS
G = SL_GROUP * T
COVER_CHUNK = COVER_THREADS * COVER_ITEMS
MAX_ANCHOR_GAP = RC._constant("walk.h", "kMaxAnchorGap")   # longer words go to the long-word kernels (steps_all / ksteps_all)
assert (SL_ITEMS, SL_GROUP, COVER_THREADS, COVER_ITEMS, STEPS_PER_MARK) == (16, 64, 1024, 8, 4)
assert (STEP_BUCKET_BITS, STEP_BUCKET_BITS_MAX, STEP_ID_BITS, STEP_MAX_LEN, BLOCK, WAVE) == (18, 21, 20, 2048, 256, 64)
assert T == 4096 and COVER_CHUNK == 8192 and KEY_BITS == 32 and MAX_ANCHOR_GAP == 2048

FOCUS = "m"


def word_of(line):
    return line[2:] if line.startswith("##") else line


def eligible(vocab):
    """lines that are marks: not special ([...]); no case here holds a malformed line"""
    return [w for w in vocab if not (len(w) > 2 and w[0] == "[" and w[-1] == "]")]


def s_string(text, vocab):
    """S of the reference layout: text . 1 . (word . 1 per line)"""
    t = text.decode("utf-8") if isinstance(text, (bytes, bytearray)) else text
    return t + "\x01" + "".join(word_of(w) + "\x01" for w in vocab)


def expected_step_stats(case, vocab_in_s, n_needed_groups=0):
    """wp_step_stats from the construction (linear_path.h, the constructor's arithmetic restated)"""
    M = len(eligible(case.vocab))
    n_text = case.n_text
    n = n_text + 1 + (sum(len(word_of(w)) + 1 for w in case.vocab) if vocab_in_s else 0)
    P = STEPS_PER_MARK * M + 1
    bucket_bits = min(STEP_BUCKET_BITS_MAX, max(STEP_BUCKET_BITS, bit_length(4 * P)))
    bs = max(0, bit_length(n) - bucket_bits)
    bsa = max(0, bit_length(n) - STEP_BUCKET_BITS)
    kb = min(KEY_BITS, max(1, bit_length(n - 1) - bs))
    kba = min(KEY_BITS, max(1, bit_length(n - 1) - bsa))
    key_lookup = 0 if (vocab_in_s or M == 0) else 1
    n_tiles = -(-n // T)
    longest = max([len(word_of(w)) for w in case.vocab] + [1])
    return dict(n_marks=M, n_steps=P + (2 * n_needed_groups if key_lookup else 0), n_tiles=n_tiles,
                n_groups_of_tiles=-(-n_tiles // SL_GROUP), bucket_shift=bs, bucket_shift_all=bsa, key_shift=KEY_BITS - kb,
                key_shift_all=KEY_BITS - kba, packed=1 if longest < STEP_MAX_LEN and len(case.vocab) < (1 << STEP_ID_BITS) else 0,
                key_lookup=key_lookup)


class Case:
    """layout "S": checked in slot space (reference layout) and, ids and statistics, on the default handle; "K": key space;
    "F": both.  claims: what test_step_cases.py proves from the oracle and the model; marks: {vocab line index: (slot, forward
    run, backward run)} for an S case."""

    def __init__(self, name, layout, text, vocab, claims=None, marks=None, families=()):
        self.name, self.layout, self.text, self.vocab = name, layout, text, list(vocab)
        self.claims, self.marks, self.families = dict(claims or {}), dict(marks or {}), list(families)
        self.n_text = len(text.decode("utf-8")) if len(text) < (1 << 22) else None
        self.heavy = False   # a vocabulary of 2^20 lines: every handle costs seconds of host time, the option matrix is left out
        assert len(vocab) == len(set(vocab)) or "dup" in name

    @property
    def low_cp(self):
        return b"\x00" in self.text or b"\x01" in self.text


CASES = {}


def case(name):
    def deco(f):
        assert name not in CASES, name
        CASES[name] = f
        return f
    return deco


# ---- family S ---------------------------------------------------------------------------------------------------------------

def _fit(tokens, core, slot, n=None, focus=FOCUS, tail=True):
    """words = core + padding in front ("a", "aa": symbols below the focus) + words of "z" behind, such that the number of
    symbols of S below `focus` is `slot` and, with a tail, S has n symbols.  Returns (text bytes, vocab, n of S)."""
    vocab = ["[UNK]"] + list(tokens)
    base = s_string(" ".join(core), vocab)
    front0, n0 = sum(1 for ch in base if ch < focus), len(base)
    d = slot - front0
    zc = 0
    if tail:
        zc = 70 if n is None else n - n0 - d
        assert zc >= 1, (slot, n, n0, d)
    j = -(-zc // 50)          # tail words: one joining blank each
    rest = d - j
    assert rest == 0 or rest >= 2, (slot, front0, j)
    y = rest % 2
    x = (rest - 3 * y) // 2
    assert x >= 0
    zs = [("z" * 50)] * (zc // 50) + (["z" * (zc % 50)] if zc % 50 else [])
    words = list(core) + ["a"] * x + ["aa"] * y + zs
    text = " ".join(words)
    S = s_string(text, vocab)
    assert sum(1 for ch in S if ch < focus) == slot and (n is None or not tail or len(S) == n), (slot, n, len(S))
    return text.encode("utf-8"), vocab, len(S)


def _s_case(name, f, b, local, tile=0, n=None, tail=True, n_mod=None, extra_claims=None):
    """token "m": f occurrences "m ", b occurrences "m<0>", the mark at local slot `local` of tile `tile`"""
    @case(name)
    def _():
        core = ["m"] * f + ["m\x00"] * b
        if not core:
            core = ["a"]
        slot = tile * T + local
        nn = n
        if n_mod is not None:   # the smallest length behind the run with that many slots in the last tile
            nn = (slot + f + 80) // T * T + n_mod
            while nn < slot + f + 80:
                nn += T
        text, vocab, n_s = _fit([FOCUS], core, slot - b, nn, tail=tail)
        end = slot + 1 + f     # first slot behind the forward run
        claims = dict(n=n_s, n_tiles=-(-n_s // T), local=local, tile=tile, fwd=f, bwd=b, fwd_end=end,
                      surv_fwd=int(end >= min((tile + 1) * T, n_s)), surv_bwd=int(slot - b <= tile * T),
                      fwd_whole_tiles=max(0, end // T - tile - 1) if end < n_s else max(0, n_s // T - tile - 1),
                      stop_tile=end // T if end < n_s else -1)
        claims.update(extra_claims or {})
        return Case(name, "S", text, vocab, claims, marks={1: (slot, f, b)})


RUNS = (0, 1, 62, 63, 64, 65, 127, 128, 129)
for _f in RUNS:
    _s_case("S_fwd_%d" % _f, _f, 0, 300 + _f)
for _b in RUNS:
    _s_case("S_bwd_%d" % _b, 3, _b, 700 + 3 * _b)
for _l, _nm in ((0, "0"), (1, "1"), (63, "63"), (64, "64"), (T - 2, "T-2"), (T - 1, "T-1")):
    _s_case("S_local_%s" % _nm, 5, 0, _l, tile=1)
_s_case("S_last_tile_1", 7, 0, 500, n_mod=1)
_s_case("S_last_tile_T-1", 7, 0, 500, n_mod=T - 1)
_s_case("S_end_last_slot", 38, 0, T - 40, tile=1)      # first slot behind the run: the tile's last
_s_case("S_end_boundary", 39, 0, T - 40, tile=1)       # ... slot 0 of the next tile: survives, popped by its first boundary
_s_case("S_end_next_1", 40, 0, T - 40, tile=1)
_s_case("S_end_n", 2 * T + 17, 0, T - 40, tile=2, tail=False)  # nothing sorts behind "m": on the stack to the end


def _tiles_case(name, w, k):
    """forward over w whole tiles from tile g * 64 + k (the smallest g with room for the blanks of the run in front)"""
    f = 9 + w * T + 5
    g = 0
    while (g * SL_GROUP + k) * T + T - 10 < f + 40:
        g += 1
    t0 = g * SL_GROUP + k
    stop = t0 + w + 1
    _s_case(name, f, 0, T - 10, tile=t0, extra_claims=dict(stop_group_delta=stop // SL_GROUP - t0 // SL_GROUP))


_tiles_case("S_tiles_1_own", 1, 3)
_tiles_case("S_tiles_1_next", 1, 63)
_tiles_case("S_tiles_2_own", 2, 3)
_tiles_case("S_tiles_2_next", 2, 62)
_tiles_case("S_tiles_63", 63, 0)
_tiles_case("S_tiles_64", 64, 0)
_tiles_case("S_tiles_65", 65, 0)
_tiles_case("S_tiles_65_two_groups", 65, 63)
_s_case("S_back_tiles_1", 3, 5 + T + 3, 5, tile=4, extra_claims=dict(bwd_whole_tiles=1))
_s_case("S_back_tiles_2", 3, 5 + 2 * T + 3, 5, tile=7, extra_claims=dict(bwd_whole_tiles=2))
_s_case("S_back_group", 3, 10, 5, tile=SL_GROUP, extra_claims=dict(bwd_group_delta=1))

FAR_F = (SL_GROUP + 1) * G + 3 * T   # the run: 65 groups and three tiles of occurrences


@case("S_far_group")
def _():
    """the mark's slot is FAR_F (the blanks of its own occurrences) plus a handful; the run ends FAR_F + 1 slots on, in a
    tile more than 64 groups behind the mark's group: the first trip of the gb += kWave loop finds no group, the second does"""
    text = b"m " * FAR_F + b"z" * 50
    vocab = ["[UNK]", FOCUS]
    front = FAR_F + 1 + 2 + 5   # blanks, the separators, "[UNK]"
    n = 2 * FAR_F + 50 + 1 + 6 + 2
    end = front + 1 + FAR_F
    c = Case("S_far_group", "S", text, vocab,
             dict(n=n, n_tiles=-(-n // T), tile=front // T, local=front % T, fwd=FAR_F, fwd_end=end, stop_tile=end // T,
                  stop_group_delta=end // G - front // G), marks={1: (front, FAR_F, 0)})
    c.n_text = 2 * FAR_F + 50
    return c


def _two(name, tokens, core, marks_of):
    @case(name)
    def _():
        text, vocab, n_s = _fit(tokens, core, 900)
        return Case(name, "S", text, vocab, dict(n=n_s), marks=marks_of(900))


# order of the suffixes that start with "m": "m<1>" (the line m), "m " x 40, "mn<1>" (the line mn), "mn " x 30, "mp " x 20
_two("S_two_nested", ["m", "mn"], ["m"] * 40 + ["mn"] * 30 + ["mp"] * 20, lambda s: {1: (s, 91, 0), 2: (s + 41, 30, 0)})
_two("S_two_same_end", ["m", "mn"], ["m"] * 40 + ["mn"] * 30, lambda s: {1: (s, 71, 0), 2: (s + 41, 30, 0)})
# ("p" and the words "pq": the symbols below "p" are those below "m", the 1 + 40 + 30 "m" and the 30 "n")
_two("S_two_disjoint", ["m", "p"], ["m"] * 40 + ["mn"] * 30 + ["p"] * 9 + ["pq"] * 8, lambda s: {1: (s, 70, 0), 2: (s + 101, 17, 0)})
# (S ends "...m<1>m<1>": the line ##m, the shorter suffix, stands first; the line m one slot on, covered from the left by it)
_two("S_both_classes", ["m", "##m"], ["m"] * 25 + ["am"] * 12 + ["amm"] * 5, lambda s: {2: (s, 48, 0), 1: (s + 1, 47, 1)})


def _dup(name, tokens):
    @case(name)
    def _():
        text, vocab, n_s = _fit(tokens, ["m"] * 70 + ["mn"] * 66 + ["amn"] * 5, 1000)
        return Case(name, "S", text, vocab, dict(n=n_s, full_depth=1))


_dup("S_dup_same_class", ["m", "mn", "m"])
_dup("S_dup_both_classes", ["m", "##m", "mn", "m", "##m"])


def _s_tokens(M):
    @case("S_tokens_%d" % M)
    def _():
        toks = ([FOCUS] + [a + b for a in "nopqrstuvwxy" for b in "nopqrst"])[:M]
        rng = random.Random(M)
        core = [rng.choice(toks) + rng.choice(["", "n", "zz"]) for _ in range(300)] if toks else ["m"] * 10
        text, vocab, n_s = _fit(toks, core, 2000)
        return Case("S_tokens_%d" % M, "S", text, vocab, dict(n=n_s, n_marks=M))


for _M in (0, 1, 63, 64, 65):
    _s_tokens(_M)


# ---- family K ---------------------------------------------------------------------------------------------------------------

WIDE = dict(zip("abcdefghijklmnopqrstuvwxyz", RC._CYRILLIC[16:42]))   # one order-preserving letter for every ASCII letter


def _widen(words, vocab):
    """the same case over Cyrillic letters (their order is the ASCII letters' order), and a word that holds more than 255
    distinct code points: 32-bit symbols"""
    tr = lambda s: "".join(WIDE.get(ch, ch) for ch in s)
    return [tr(w) for w in words] + [RC.WIDE_FILL], [w if w == "[UNK]" else tr(w) for w in vocab]


def _strings(count, first="b", letters="cdefg"):
    """`count` distinct words in lexicographic order: `first`, then first + every string over `letters`, short ones first"""
    out, layer = [first], [first]
    while len(out) < count:
        layer = [w + ch for w in layer for ch in letters]
        out += layer
    return sorted(out[:count])


def _k_case(name, words, vocab, claims=None, seed=0, last=None, families=(), wide=False, shuffle=True):
    rng = random.Random(seed)
    words = list(words)
    if shuffle:
        rng.shuffle(words)
    if last is not None:
        words.append(last)
    if wide:
        words, vocab = _widen(words, vocab)
        if last is not None:
            words.append(words.pop(len(words) - 2))   # (the filler word stays in front of the last word)
    text = " ".join(words).encode("utf-8")
    c = Case(name, "K", text, vocab, dict(claims or {}), families=families)
    c.claims.setdefault("n_marks", len(eligible(vocab)))
    c.claims.setdefault("n_total", c.n_text + 1)
    return c


def _marks_vocab(M, first="b"):
    """M eligible lines, both classes interleaved in lexicographic order: the words alternate prefix-class, ##-class, both"""
    lines, i = [], 0
    ws = _strings(M, first)
    for w in ws:
        kinds = (("",), ("##",), ("", "##"))[i % 3] if w != first else ("", "##")
        for kd in kinds:
            if len(lines) < M:
                lines.append(kd + w)
        i += 1
        if len(lines) >= M:
            break
    assert len(lines) == M
    return lines


def _k_marks(M, wide=False):
    name = ("K_wide_marks_%d" if wide else "K_marks_%d") % M

    @case(name)
    def _():
        lines = _marks_vocab(M)
        ws = sorted({word_of(w) for w in lines})
        rng = random.Random(M)
        # words of the vocabulary, glued pairs (in-word positions), and "bz" / "cbz": the first token ("b", mark 0 or 1)
        # is the longest match at slots behind every other mark
        words = [rng.choice(ws) for _ in range(1500)] + [rng.choice(ws) + rng.choice(ws) for _ in range(700)]
        words += ["bz"] * 9 + ["cbz"] * 9 + ["b"] * 5 + ws[-3:] * 3
        return _k_case(name, words, ["[UNK]"] + lines, dict(cover="b", word="bz", between=M - 2), seed=M, wide=wide)


for _M in (63, 64, 65, 4096, 4097, COVER_CHUNK - 1, COVER_CHUNK, COVER_CHUNK + 1, 2 * COVER_CHUNK + 1):
    _k_marks(_M)
_k_marks(COVER_CHUNK + 1, wide=True)


def _k_cover(k, other, occur=True, name=None, wide=False):
    name = name or "K_cover_%d_%s" % (k, "other" if other else "same")

    @case(name)
    def _():
        mids = _strings(k, "ab", "bcd")           # k words between "a" and "az"
        lines = ["a", "##a"] + [("##" if other else "") + w for w in mids]
        words = ["az"] * 6 + ["aaz"] * 6 + ["a"] * 3 + ["aa"] * 2
        if occur:   # every third of the k tokens occurs, at a word's start and inside a word
            for w in mids[::3]:
                words += [w, "a" + w, w + "z"]
        return _k_case(name, words, ["[UNK]"] + lines, dict(cover="a", word="az", between=k, same_class=0 if other else 1),
                       seed=k, wide=wide)


for _k in (1, 63, 64, 65, 129):
    _k_cover(_k, False)
    _k_cover(_k, True)
for _k in (1, 64, 65):
    _k_cover(_k, False, occur=False, name="K_empty_%d" % _k)
_k_cover(65, True, wide=True, name="K_wide_cover_65")


def _k_chain(name, wide=False):
    @case(name)
    def _():
        stem = "hijklmn"
        lines = [kd + stem[:d] for d in range(1, 8) for kd in ("", "##")]
        words = []
        for d in range(1, 8):   # words leave the chain at every depth: at the end, with a symbol below, with one above
            for tail_ in ("", "a", "z", "zz"):
                words += [stem[:d] + tail_, "z" + stem[:d] + tail_, "h" + stem[:d] + tail_]
        return _k_case(name, words * 2, ["[UNK]"] + lines, dict(chain=7), wide=wide)


_k_chain("K_chain")
_k_chain("K_wide_chain", wide=True)


def _k_ends(name, tok, filler, last):
    @case(name)
    def _():
        words = [tok] * 4 + [tok + x for x in filler] * 3 + [f for f in filler] * 5
        return _k_case(name, words, ["[UNK]", tok, "##" + tok] + [f for f in filler] + ["##" + f for f in filler],
                       dict(end_token=tok, last_word=last), last=last)


# "a" is the smallest symbol of the text: the range of the token "a" starts at the first slot that holds a non-blank
_k_ends("K_first_slot_token", "a", ["c", "d", "e"], "a")
_k_ends("K_first_slot_prefix", "a", ["c", "d", "e"], "ac")
# "z" is the largest: its range ends at n, and "zy", the largest key of all, is the last word or not
_k_ends("K_last_slot_token", "z", ["c", "d", "y"], "z")
_k_ends("K_last_slot_prefix", "z", ["c", "d", "y"], "zy")


def _exact_text(rng, ws, n_text, last=None):
    """words of ws joined by blanks, exactly n_text code points"""
    out, size = [], 0
    tail_ = (" " + last) if last else ""
    while True:
        w = rng.choice(ws)
        room = n_text - len(tail_) - size - (1 if out else 0)
        if room <= 12:
            break
        out.append(w)
        size += len(w) + (1 if len(out) > 1 else 0)
    room = n_text - len(tail_) - size - 1
    out.append("c" * room)
    text = " ".join(out) + tail_
    assert len(text) == n_text
    return text


def _k_n(n_total):
    @case("K_n_%d" % n_total)
    def _():
        lines = _marks_vocab(40)
        ws = sorted({word_of(w) for w in lines}) + ["bz", "cb"]
        text = _exact_text(random.Random(n_total), ws, n_total - 1)
        c = Case("K_n_%d" % n_total, "K", text.encode(), ["[UNK]"] + lines, dict(n_marks=40, n_total=n_total))
        return c


for _n in ((1 << 18) - 1, 1 << 18, (1 << 18) + 1, (1 << 19) + 1):
    _k_n(_n)


def _k_shift_all(M):
    @case("K_shift_all_%d" % M)
    def _():
        lines = _marks_vocab(M)
        ws = sorted({word_of(w) for w in lines})
        rng = random.Random(M)
        long_word = "".join(rng.choice(ws) for _ in range(900))   # tokenisable, more than kMaxAnchorGap positions
        assert len(long_word) > MAX_ANCHOR_GAP + 100
        head = " ".join(rng.choice(ws) for _ in range(3000)) + " " + long_word + " "
        text = head + _exact_text(rng, ws + ["bz"], (1 << 19) + 4000 - len(head))
        return Case("K_shift_all_%d" % M, "K", text.encode(), ["[UNK]"] + lines,
                    dict(n_marks=M, n_total=len(text) + 1, shifts_differ=int(M >= 16384), long_words=1))


# bit_length(4 * (4 M + 1)) passes kStepBucketBits = 18 between M = 16383 and 16384
assert bit_length(4 * (4 * 16383 + 1)) == STEP_BUCKET_BITS and bit_length(4 * (4 * 16384 + 1)) == STEP_BUCKET_BITS + 1
_k_shift_all(16383)
_k_shift_all(16384)


def _flat_strings(count, letters):
    """`count` distinct words over `letters` in lexicographic order, short ones first"""
    out, layer = [], [""]
    while len(out) < count:
        layer = [w + ch for w in layer for ch in letters]
        out += layer
    return sorted(out[:count])


def _k_pack(lines_total):
    """a vocabulary of `lines_total` lines ("[UNK]" among them): below 2^kStepIdBits lines a step value carries the token's
    length above its id, from 2^kStepIdBits lines on it does not (tokens of at most five symbols over seventeen letters: no
    token outgrows a key)"""
    @case("K_pack_%d" % lines_total)
    def _():
        ws = _flat_strings(lines_total - 1, "cdefghijklmnopqrs")
        rng = random.Random(lines_total)
        pick = [rng.choice(ws) for _ in range(4000)]
        words = pick[:2500] + [a + b for a, b in zip(pick[2500:3200], pick[3200:3900])] + [w + "z" for w in pick[3900:]]
        c = _k_case("K_pack_%d" % lines_total, words, ["[UNK]"] + ws, dict(packed=int(lines_total < (1 << STEP_ID_BITS))))
        c.heavy = True
        return c


_k_pack((1 << STEP_ID_BITS) - 1)
_k_pack(1 << STEP_ID_BITS)


@case("K_with_family")
def _():
    """a refine_cases.Family (tokens longer than a key, a needed group of 65 members) beside a K vocabulary: the group's
    two starts join the step list, and the key-space table answers kStepNeeded for its key"""
    fam = RC.Family("T", at=[RC.BASE + 1, RC.BASE + 4], k=65)
    lines = _marks_vocab(64)
    ws = sorted({word_of(w) for w in lines})
    rng = random.Random(5)
    words = [rng.choice(ws) for _ in range(400)] + ["bz"] * 5 + fam.members
    used = sorted(set("".join(fam.members)))
    vocab = ["[UNK]"] + lines + [ch for ch in used if ch not in lines] + ["##" + ch for ch in used] + fam.tokens
    return _k_case("K_with_family", words, vocab, dict(n_needed_groups=1), families=[fam])


# ---- family F: seeded compositions ---------------------------------------------------------------------------------------------
F_SEEDS = 48


def _composed(seed):
    rng = random.Random(9000 + seed)
    sym = "bcde"[:rng.choice([3, 4])]
    nv = rng.choice([3, 8, 20, 70, 130])
    words = set()
    while len(words) < nv:
        words.add("".join(rng.choice(sym) for _ in range(rng.randint(1, 6))))
    lines = []
    for w in sorted(words):
        kd = rng.choice(["", "", "##", "both"])
        lines += ([w] if kd in ("", "both") else []) + (["##" + w] if kd in ("##", "both") else [])
    rng.shuffle(lines)
    n_text = rng.choice([T - 200, T + 1, 2 * T - 1, 2 * T + 300, 3 * T - 5])
    text, size = [], 0
    while size < n_text:
        w = "".join(rng.choice(sym) for _ in range(rng.randint(1, 9)))
        text.append(w)
        size += len(w) + 1
    t = " ".join(text)
    if seed % 6 == 5:   # a low code point: the default handle takes the reference layout
        t = t[:len(t) // 2] + "\x00" + t[len(t) // 2:]
    return Case("F_%03d" % seed, "F", t.encode(), ["[UNK]"] + lines)


for _s in range(F_SEEDS):
    CASES["F_%03d" % _s] = functools.partial(_composed, _s)


def names(groups="SK"):
    return [n for n in CASES if n[0] in groups]


BIG = ("S_far_group",)   # its own tests: ids only


@functools.lru_cache(maxsize=6)
def build(name):
    c = CASES[name]()
    c.name = name
    return c


def between_text(case_):
    """a text of another population for the same vocabulary, encoded between two encodes of a case: other words, another
    length (more than a tile more), another first and last word"""
    ws = sorted({word_of(w) for w in eligible(case_.vocab)}) or ["m"]
    rng = random.Random(len(case_.vocab))
    return " ".join(["zq"] + [rng.choice(ws) + rng.choice(["", "q", ws[0]]) for _ in range(T + 700)] + ["q"]).encode("utf-8")


# two K cases and two S cases, embedded in the middle and at the end of 2.4 MB of English words
EMBEDDED = ["K_cover_65_other", "K_chain", "S_bwd_65", "S_two_nested"]
