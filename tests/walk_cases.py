"""Inputs placed on the thresholds of the walk (csrc/walk.h, csrc/fast.h, the host side in linear_path.h::walk and
fast_path.h), shared by test_walk_cases.py (no GPU) and test_gpu_walk_edges.py: the constants, read from the headers by
name; a Python model of the class rule (class of a code point, hard / soft from the vocabulary, anchors, stretches, the
gap as the gap kernels measure it) that says which variant of the walk an input reaches; vocabulary families; and the
cases, in groups W (wide walk), L (long words), S (staging and rollback), B (dealing and lists), A (anchor tiles and
windows), C (coverage rule) and F (seeded composition).

build(name) -> (text as UTF-8 bytes, vocabulary lines, expect).  expect["linear"] / expect["fast"] are the model's
statistics of the default handle (wp_stats.anchor_mode / staged_emit / n_anchors and wp_walk_stats; "fast" is None where
the fast entry point is not compared), expect["claims"] what the builder says it built — test_walk_cases.py holds the model
to the claims, test_gpu_walk_edges.py holds the library to the model.  Importing this module loads no library."""
import os
import random
import re

from bruteforce import is_punct, is_space, is_spacing

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "wordpiece_amd", "csrc")


def _constant(header, name):
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(r"^constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, f.read(), re.M)
    assert m, (header, name)
    return int(m.group(1))


# ---- the constants the cases stand on: a changed constant moves the cases with it
WIDE_MIN = _constant("walk.h", "kWideMin")          # a stretch longer than this goes to a whole wave
WIDE_PER_LANE = _constant("walk.h", "kWidePerLane")
MAX_GAP = _constant("walk.h", "kMaxAnchorGap")      # longer: pointer doubling (hard vocabularies) / the coverage rule
STAGE_IDS = _constant("walk.h", "kStageIds")        # ids of a word kept in LDS; the rest spill
WB_PER_WAVE = _constant("walk.h", "kWbPerWave")
ANCHOR_BYTES = _constant("walk.h", "kAnchorBytes")
BLOCK = _constant("common.h", "kBlock")
WAVE = _constant("common.h", "kWave")
WIDE_WINDOW = WAVE * WIDE_PER_LANE                  # walk.h, kWideWindow
WB_WORDS = WB_PER_WAVE * (BLOCK // WAVE)            # walk.h, kWbWords: words per workgroup of the list-building walks
ANCHOR_TILE = BLOCK * ANCHOR_BYTES                  # walk.h, kAnchorTile
REACH_TILE = BLOCK * 8                              # walk.h, kReachTile
LEAN_MAX_LEN = ANCHOR_BYTES - 1                     # walk_lean_kernel: the straight step is taken for len < 15 (or at the end)
assert REACH_TILE <= MAX_GAP and WIDE_WINDOW == 256 and STAGE_IDS >= 2

LET = "abcdefg"   # the letters every family knows, alone and as ## pieces
FAIL = "h"        # known to the plain families, unknown to the "minus" ones: where it stands, the word fails
CJK = "中文"


# ---- vocabulary families ------------------------------------------------------------------------------------------------

def tok(n):
    """the piece of exactly n symbols (letters no other token uses; a shorter piece is a prefix of a longer one)"""
    return ("rstuvwxyz" * 3)[:n]


def single(minus=False, unk=True, comma=True):
    """single-character pieces over a small alphabet, all with ## forms (minus: without FAIL)"""
    letters = LET + ("" if minus else FAIL)
    return (["[UNK]"] if unk else []) + list(letters) + ["##" + c for c in letters] + ([","] if comma else []) + ["."]


def pieces(minus=False):
    """single() and pieces of exactly 14, 15, 16 and 17 symbols, and a two-symbol piece"""
    v = single(minus) + ["pq", "##pq"]
    for n in (14, 15, 16, 17):
        v += [tok(n), "##" + tok(n)]
    return v


def soft(minus=False):
    """pieces() and tokens that make spacing chars soft: a blank inside, ',' inside, multi-character CJK tokens.
    '.' stays hard."""
    return pieces(minus) + ["x y", "x,y", "中文", "中文中", "中", "文", "##文", "##中"]


def with_cjk(minus=False):
    """single() and one CJK char as a token of its own: every spacing char stays hard"""
    return single(minus) + ["中"]


# ---- the model ------------------------------------------------------------------------------------------------------------

def parse_vocab(vocab):
    """-> (eligible tokens as (is_prefix, code points), id of [UNK] or -1), utils.cpp:81-121"""
    toks, unk = [], -1
    for i, w in enumerate(vocab):
        if w == "[UNK]":
            unk = i
        cps, prefix, special = [ord(c) for c in w], True, False
        if len(cps) >= 2 and cps[0] == 35 and cps[1] == 35:
            prefix, cps = False, cps[2:]
        elif len(cps) > 2 and cps[0] == 91 and cps[-1] == 93:
            special = True
        malformed = len(cps) > 1 and all(is_punct(c) or is_space(c) for c in cps)
        if not special and not malformed:
            toks.append((prefix, cps))
    return toks, unk


class Model:
    """Which variant of the walk the default handle takes for (text, vocab), from the class rule alone."""

    def __init__(self, text, vocab):
        cps = [ord(c) for c in text]
        toks, self.unk = parse_vocab(vocab)
        # a spacing char is soft when it occurs inside an eligible token of more than one symbol (vocab.h, derive)
        self.soft = {c for _, w in toks if len(w) > 1 for c in w if is_spacing(c)}
        self.all_hard = not self.soft
        self.n = len(cps)
        self.space = [is_space(c) for c in cps]
        self.spacing = [is_spacing(c) for c in cps]
        self.punct = [is_punct(c) for c in cps]
        self.hard = [s and c not in self.soft for s, c in zip(self.spacing, cps)]

    def _to_blank(self, lo, hi):
        """a distance above MAX_GAP as the gap and collect kernels measure it: up to the first blank, at most MAX_GAP + 1"""
        q, stop = lo, min(hi, lo + MAX_GAP + 1)
        while q < stop and not self.space[q]:
            q += 1
        return q - lo

    def linear_anchors(self):
        sp, hd = self.space, self.hard
        return [p for p in range(self.n) if not sp[p] and (p == 0 or hd[p] or hd[p - 1])]

    def stretches(self, anchors):
        """[anchor, next anchor) for every anchor; the last one runs to the end of the text"""
        return list(zip(anchors, anchors[1:] + [self.n]))

    def linear(self):
        anchors = self.linear_anchors()
        st = self.stretches(anchors)
        gap = 0
        for k in range(len(anchors) + 1):  # anchor_gap_kernel: the text start and end included
            hi = anchors[k] if k < len(anchors) else self.n
            lo = anchors[k - 1] if k else 0
            d = hi - lo
            if d > MAX_GAP and self.all_hard:
                d = self._to_blank(lo, hi)
            gap = max(gap, d)
        out = dict(anchor_mode=0, staged_emit=0, lean=0, n_wide_words=0, n_long_words=0, max_anchor_gap=gap,
                   n_anchors=len(anchors))
        if self.all_hard and gap > MAX_GAP:      # long words by pointer doubling, ids through the per-position array
            out["n_long_words"] = sum(1 for lo, hi in st if hi - lo > MAX_GAP and self._to_blank(lo, hi) > MAX_GAP)
            out["anchor_mode"] = 2 if out["n_long_words"] else 0
        elif gap > MAX_GAP:                      # soft spacing chars: the coverage rule, lists again
            out.update(anchor_mode=1, staged_emit=1, lean=1, n_anchors=None)
        elif self.all_hard:                      # class rule, one word per stretch: lists, and the wide walk
            out.update(staged_emit=1, lean=1)
            if gap > WIDE_MIN:
                out["n_wide_words"] = sum(1 for lo, hi in st if hi - lo > WIDE_MIN)
        return out

    def fast_anchors(self):
        sp, sc, pu = self.space, self.spacing, self.punct
        return [p for p in range(self.n) if not sp[p] and (p == 0 or sc[p] or sp[p - 1] or pu[p - 1])]

    def fast(self):
        anchors = self.fast_anchors()
        st = self.stretches(anchors)
        gap = 0
        for lo, hi in st:  # fast_anchor_gap_kernel: from an anchor on
            d = hi - lo
            if d > MAX_GAP:
                d = self._to_blank(lo, hi)
            gap = max(gap, d)
        out = dict(anchor_mode=0, staged_emit=1 if gap <= MAX_GAP else 0, lean=0, n_wide_words=0, n_long_words=0,
                   max_anchor_gap=gap, n_anchors=len(anchors))
        if gap > MAX_GAP:  # (a CJK char and the run behind it stay with their lane)
            out["n_long_words"] = sum(1 for lo, hi in st if hi - lo > MAX_GAP and self._to_blank(lo, hi) > MAX_GAP
                                      and not self.spacing[lo])
            out["anchor_mode"] = 2 if out["n_long_words"] else 0
        return out


# ---- texts ------------------------------------------------------------------------------------------------------------------

def word(n, fail_at=(), start=0):
    """n letters of LET in turn (as many ids under single()), FAIL at the given positions"""
    w = [LET[(start + i) % len(LET)] for i in range(n)]
    for p in fail_at:
        w[p] = FAIL
    return "".join(w)


def para(n):
    """n CJK chars in a row"""
    return (CJK * (n // 2 + 1))[:n]


CASES = {}   # name -> (builder, fast applies)


def case(name, fast=True):
    def deco(f):
        assert name not in CASES, name
        CASES[name] = (f, fast)
        return f
    return deco


def _add(name, text, vocab, fast=True, **claims):
    """a case whose text is known here; claims: lin_* / fast_* statistics, n_ids, longest (stretch under the class rule)"""
    assert name not in CASES, name
    CASES[name] = (lambda: (text, vocab, claims), fast)


D3 = (-1, 0, 1)
WIDE = dict(lin_anchor_mode=0, lin_staged_emit=1, lin_lean=1, lin_n_long_words=0)   # lists, the wide walk ran or could have
LONG = dict(lin_anchor_mode=2, lin_staged_emit=0, lin_lean=0, lin_n_wide_words=0, fast_anchor_mode=2, fast_staged_emit=0)

# ---- W: the wide walk ----------------------------------------------------------------------------------------------------------
for d in D3:  # a stretch around kWideMin, made three ways
    n = WIDE_MIN + d
    wide = 1 if n > WIDE_MIN else 0
    _add("W_stretch_blank%+d" % d, "ab " + word(n - 1) + " ab", single(), longest=n, lin_n_wide_words=wide, lin_max_anchor_gap=n, **WIDE)
    _add("W_stretch_punct%+d" % d, "ab " + word(n) + ",ab", single(), longest=n, lin_n_wide_words=wide, lin_max_anchor_gap=n, **WIDE)
    _add("W_stretch_blanks%+d" % d, "ab " + word(10) + " " * (n - 10) + "ab", single(), longest=n, lin_n_wide_words=wide,
         lin_max_anchor_gap=n, n_ids=2 + 10 + 2, **WIDE)
for n0 in (WAVE, WIDE_WINDOW, 2 * WIDE_WINDOW):  # word length around the end search's 64 and the window's 256
    for d in D3:
        _add("W_len_%d%+d" % (n0, d), "ab " + word(n0 + d) + " ab", single(), longest=n0 + d + 1, lin_n_wide_words=1,
             n_ids=n0 + d + 4, **WIDE)
for d in D3:  # kMaxAnchorGap: MAX_GAP letters and a blank are a stretch of MAX_GAP + 1 and a gap of MAX_GAP: wide, not long
    n = MAX_GAP + d
    if d <= 0:
        _add("W_len_max%+d_blank" % d, "ab " + word(n) + " ab", single(), longest=n + 1, lin_n_wide_words=1, lin_max_anchor_gap=MAX_GAP,
             n_ids=n + 4, fast_staged_emit=1, fast_max_anchor_gap=MAX_GAP, **WIDE)  # (MAX_GAP - 1 letters and the blank: the stretch)
        _add("W_len_max%+d_punct" % d, "ab " + word(n) + ",ab", single(), longest=n, lin_n_wide_words=1, lin_max_anchor_gap=n,
             n_ids=n + 5, fast_staged_emit=1, **WIDE)
    else:
        _add("W_len_max%+d_blank" % d, "ab " + word(n) + " ab", single(), longest=n + 1, lin_n_long_words=1,
             lin_max_anchor_gap=MAX_GAP + 1, fast_n_long_words=1, n_ids=n + 4, **LONG)
        _add("W_len_max%+d_punct" % d, "ab " + word(n) + ",ab", single(), longest=n, lin_n_long_words=1, fast_n_long_words=1,
             n_ids=n + 5, **LONG)
# a token against the window's end and the word's end ("pq" is the only two-symbol piece)
_add("W_token_ends_on_window", "ab " + word(WIDE_WINDOW - 2) + "pq" + word(100) + " ab", pieces(), lin_n_wide_words=1,
     n_ids=2 + WIDE_WINDOW - 2 + 1 + 100 + 2, **WIDE)
_add("W_token_straddles_window", "ab " + word(WIDE_WINDOW - 1) + "pq" + word(100) + " ab", pieces(), lin_n_wide_words=1,
     n_ids=2 + WIDE_WINDOW - 1 + 1 + 100 + 2, **WIDE)
_add("W_token_starts_next_window", "ab " + word(WIDE_WINDOW) + "pq" + word(100) + " ab", pieces(), lin_n_wide_words=1,
     n_ids=2 + WIDE_WINDOW + 1 + 100 + 2, **WIDE)
_add("W_token_ends_on_word", "ab " + word(298) + "pq ab", pieces(), lin_n_wide_words=1, n_ids=2 + 298 + 1 + 2, **WIDE)
_add("W_token_ends_on_word_window", "ab " + word(2 * WIDE_WINDOW - 2) + "pq ab", pieces(), lin_n_wide_words=1,
     n_ids=2 + 2 * WIDE_WINDOW - 2 + 1 + 2, **WIDE)
_add("W_long_token_straddles_window", "ab " + word(WIDE_WINDOW - 9) + tok(17) + word(30) + " ab", pieces(), lin_n_wide_words=1,
     n_ids=2 + WIDE_WINDOW - 9 + 1 + 30 + 2, **WIDE)
for where, at in (("first", 0), ("last", 399), ("second_window", 300), ("pos255", WIDE_WINDOW - 1), ("pos256", WIDE_WINDOW)):
    _add("W_break_" + where, "ab " + word(400, (at,)) + " ab", single(minus=True), lin_n_wide_words=1, n_ids=5, **WIDE)
_add("W_break_last_of_window_word", "ab " + word(WIDE_WINDOW, (WIDE_WINDOW - 1,)) + " ab", single(minus=True), lin_n_wide_words=1,
     n_ids=5, **WIDE)
for blanks in (WAVE - 1, WAVE, WAVE + 1, 200):  # the end search from the back, 64 positions at a time
    _add("W_trailing_%d" % blanks, "ab " + word(2 * WAVE) + " " * blanks + "ab", single(), longest=2 * WAVE + blanks,
         lin_n_wide_words=1, n_ids=2 * WAVE + 4, **WIDE)
    _add("W_trailing_%d_at_end" % blanks, "ab " + word(2 * WAVE) + " " * blanks, single(), lin_n_wide_words=1, n_ids=2 * WAVE + 2,
         **WIDE)
for ids in (WIDE_WINDOW - 1, WIDE_WINDOW, WIDE_WINDOW + 1, 600):  # the copy loop: kC * kWave = 256 ids per trip
    _add("W_ids_%d" % ids, "ab " + word(ids) + " ab", single(), lin_n_wide_words=1, n_ids=ids + 4, **WIDE)
# words 0 and 4 of a workgroup share a copy trip (two words per trip, kBlock / kWave = 4 apart): 300 and 70 ids
_add("W_copy_trip_unlike", word(300) + " ab ab ab " + word(70) + " ab", single(), lin_n_wide_words=2, n_ids=300 + 6 + 70 + 2, **WIDE)
_add("W_copy_trip_unlike_swapped", word(70) + " ab ab ab " + word(300) + " ab", single(), lin_n_wide_words=2, n_ids=300 + 6 + 70 + 2,
     **WIDE)
_add("W_workgroup_all_wide", " ".join(word(WIDE_MIN + 1 + k % 3, start=k) for k in range(WB_WORDS + 6)), single(),
     lin_n_wide_words=WB_WORDS + 6, **WIDE)
_add("W_first_stretch", word(100) + " ab", single(), lin_n_wide_words=1, n_ids=102, **WIDE)
_add("W_last_stretch", "ab " + word(100), single(), lin_n_wide_words=1, n_ids=102, **WIDE)
_add("W_last_stretch_blank", "ab " + word(100) + " ", single(), lin_n_wide_words=1, n_ids=102, **WIDE)
_add("W_only_stretch", word(100), single(), lin_n_wide_words=1, n_ids=100, **WIDE)
_add("W_last_stretch_unk", "ab " + word(100, (99,)), single(minus=True), lin_n_wide_words=1, n_ids=3, **WIDE)
# dense: the ids of the word fill its stretch of the scratch array exactly
_add("W_dense", "ab " + word(MAX_GAP) + ",ab", single(), longest=MAX_GAP, lin_n_wide_words=1, n_ids=MAX_GAP + 5, **WIDE)
_add("W_dense_at_end", "ab," + word(MAX_GAP), single(), longest=MAX_GAP, lin_n_wide_words=1, n_ids=MAX_GAP + 3, **WIDE)
_add("W_dense_two", word(MAX_GAP) + "," + word(MAX_GAP, start=3) + ",", single(), longest=MAX_GAP, lin_n_wide_words=2,
     n_ids=2 * MAX_GAP + 2, **WIDE)
_add("W_no_unk", "ab " + word(100, (50,)) + " ab " + word(60), single(minus=True, unk=False), lin_n_wide_words=2,
     n_ids=2 + 1 + 2 + 60, **WIDE)

# ---- L: long words ----------------------------------------------------------------------------------------------------------
for d in D3:
    n = MAX_GAP + d
    for tail_name, tail in (("blank", " ab"), ("punct", ",ab"), ("blanks3000", " " * 3000 + "ab"), ("end", "")):
        cl = dict(LONG, lin_n_long_words=1, fast_n_long_words=1) if d > 0 else dict(WIDE, lin_n_wide_words=1, fast_n_long_words=0)
        _add("L_run%+d_%s" % (d, tail_name), "ab " + word(n) + tail, single(), n_ids=2 + n + (len(tail.strip()) if tail else 0), **cl)
for k in (12, 15):  # the doubling loop runs while reach < longest
    for d in D3:
        n = (1 << k) + d
        _add("L_pow%d%+d" % (k, d), "ab " + word(n - 1) + " ab", single(), longest=n, lin_n_long_words=1, n_ids=n - 1 + 4, **LONG)
        _add("L_pow%d%+d_tokens" % (k, d), "ab " + (tok(17) + "pq" + word(9)) * ((n - 1) // 28) + word((n - 1) % 28) + " ab", pieces(),
             longest=n, lin_n_long_words=1, n_ids=11 * ((n - 1) // 28) + (n - 1) % 28 + 4, **LONG)
for where, at in (("first", 0), ("middle", 1500), ("last", 2999)):
    _add("L_fail_" + where, "ab " + word(3000, (at,)) + " ab", single(minus=True), lin_n_long_words=1, fast_n_long_words=1, n_ids=5, **LONG)
_add("L_fail_no_unk", "ab " + word(3000, (1500,)) + " ab", single(minus=True, unk=False), lin_n_long_words=1, n_ids=5, **LONG)
_add("L_several", "ab " + word(2500) + " cd " + word(100) + " " + word(3000, start=2) + " " + word(60) + " " + word(2100) + " ef,"
     + word(2300, (7,)) + " g", single(minus=True), lin_n_long_words=4, fast_n_long_words=4, n_ids=2 + 2500 + 2 + 100 + 3000 + 60 + 2100 + 2 + 1 + 1 + 1,
     **LONG)
_add("L_next_to_max_word", "ab " + word(2500) + " " + word(MAX_GAP) + " ab " + word(MAX_GAP) + ",ab", single(), lin_n_long_words=1,
     fast_n_long_words=1, n_ids=2 + 2500 + 2 * MAX_GAP + 2 + 1 + 2, **LONG)
_add("L_after_punct", "ab," + word(2500) + " ab", single(), lin_n_long_words=1, fast_n_long_words=1, n_ids=2 + 1 + 2500 + 2, **LONG)
_add("L_two_abut", word(2100) + "," + word(2200) + ",", single(), lin_n_long_words=2, fast_n_long_words=2, n_ids=4302, **LONG)
# fast: a CJK char and the run behind it are one segment chain of one lane (no word-prefix position is skipped); Linear
# stands on the position behind the CJK char as on any anchor
_add("L_fast_cjk_run", "ab 中" + word(3000) + " ab", with_cjk(), lin_n_long_words=1, fast_n_long_words=0, fast_anchor_mode=0,
     fast_staged_emit=0, fast_max_anchor_gap=MAX_GAP + 1, n_ids=2 + 1 + 3000 + 2, lin_anchor_mode=2)
_add("L_fast_cjk_run_fail", "ab 中" + word(3000, (2000,)) + " ab", with_cjk(minus=True), lin_n_long_words=1, fast_n_long_words=0,
     fast_anchor_mode=0, n_ids=2 + 1 + 1 + 2)
_add("L_fast_cjk_and_long", "ab 中" + word(3000) + " " + word(2500) + " ab", with_cjk(), lin_n_long_words=2, fast_n_long_words=1,
     fast_anchor_mode=2)

# ---- S: staging and rollback ---------------------------------------------------------------------------------------------------
LEANC = dict(lin_anchor_mode=0, lin_staged_emit=1, lin_lean=1, lin_n_wide_words=0, lin_n_long_words=0)
for d in D3:
    k = STAGE_IDS + d
    _add("S_tokens%+d" % d, "ab " + word(k) + " ab," + word(k) + "," + word(k), single(), n_ids=4 + 3 * k + 2, **LEANC)
    _add("S_tokens%+d_fail" % d, "ab " + word(k) + FAIL + " ab," + word(k) + FAIL + "," + word(k) + FAIL, single(minus=True),
         n_ids=4 + 3 + 2, **LEANC)
    _add("S_tokens%+d_fail_no_unk" % d, "ab " + word(k) + FAIL + " ab", single(minus=True, unk=False), n_ids=5, **LEANC)
_add("S_lean_max", "ab " + word(WIDE_MIN) + ",ab " + word(WIDE_MIN - 1) + " ab", single(), longest=WIDE_MIN, n_ids=2 + 2 * WIDE_MIN - 1 + 5,
     lin_max_anchor_gap=WIDE_MIN, **LEANC)
_add("S_lean_max_fail", "ab " + word(WIDE_MIN, (WIDE_MIN - 1,)) + ",ab", single(minus=True), longest=WIDE_MIN, n_ids=6, **LEANC)
for k in (3, 4, 6):  # fast: the CJK char's id stays (the mark is 1), the word behind it goes
    _add("S_fast_cjk_%d_fail" % k, "ab 中" + word(k) + FAIL + " ab", with_cjk(minus=True), n_ids=2 + 1 + 1 + 2, **LEANC)
    _add("S_fast_cjk_%d" % k, "ab 中" + word(k) + " ab", with_cjk(minus=True), n_ids=2 + 1 + k + 2, **LEANC)
COVER = dict(lin_anchor_mode=1, lin_staged_emit=1, lin_lean=1, lin_n_wide_words=0, lin_n_long_words=0)
for m in (STAGE_IDS - 1, STAGE_IDS, STAGE_IDS + 1):  # coverage rule: a stretch of several words, m ids before the mark
    for t in (1, STAGE_IDS, STAGE_IDS + 1):
        _add("S_cover_m%d_t%d" % (m, t), "." + word(m) + " " + word(t) + FAIL + " ab." + para(MAX_GAP + 52) + ".ab", soft(minus=True),
             fast=False, **COVER)
        _add("S_class_m%d_t%d" % (m, t), "." + word(m) + " " + word(t) + FAIL + " ab.ab", soft(minus=True), fast=False,
             lin_anchor_mode=0, lin_staged_emit=0, lin_lean=0, n_ids=1 + m + 1 + 2 + 1 + 2)

# ---- B: dealing and lists ------------------------------------------------------------------------------------------------------
for n0 in (WAVE, WB_PER_WAVE, WB_WORDS, 2 * WB_WORDS):
    for d in D3:
        _add("B_anchors_%d%+d" % (n0, d), " ".join(word(1 + k % 3, start=k) for k in range(n0 + d)), single(), lin_n_anchors=n0 + d,
             fast_n_anchors=n0 + d, **LEANC)
for k in (1, 2):  # every position an anchor with one id: the lists of neighbouring workgroups abut
    for d in D3:
        n = WB_WORDS * k + d
        _add("B_punct_%d%+d" % (WB_WORDS * k, d), "," * n, single(), lin_n_anchors=n, lin_max_anchor_gap=1, n_ids=n, **LEANC)
        _add("B_punct_unk_%d%+d" % (WB_WORDS * k, d), "," * n, single(comma=False), lin_n_anchors=n, n_ids=n, **LEANC)
        _add("B_punct_no_unk_%d%+d" % (WB_WORDS * k, d), "," * n, single(comma=False, unk=False), lin_n_anchors=n, n_ids=n, **LEANC)
_add("B_punct_mixed", (",a" * WB_WORDS)[:2 * WB_WORDS - 1] + ",,,", single(), lin_n_anchors=2 * WB_WORDS + 2, n_ids=2 * WB_WORDS + 2, **LEANC)


# ---- A: anchor tiles and windows -------------------------------------------------------------------------------------------------
def _prose(seed, n, fail=False):
    """n symbols of short words, blanks and punctuation"""
    rng = random.Random(seed)
    parts, size = [], 0
    while size < n + 16:
        w = word(rng.randint(1, 9), start=rng.randint(0, 6)) + (FAIL if fail and rng.random() < 0.1 else "")
        sep = rng.choice([" ", " ", " ", ",", ", ", "  ", "."])
        parts.append(w + sep)
        size += len(w) + len(sep)
    return "".join(parts)[:n]


for n0 in (ANCHOR_TILE, 2 * ANCHOR_TILE):  # n % 16 in {15, 0, 1}: the scalar tail of the 16-byte load
    for d in D3:
        _add("A_text_%d%+d" % (n0, d), _prose(n0 + d, n0 + d), single(), **LEANC)
        _add("A_text_%d%+d_anchor_last" % (n0, d), _prose(n0 + d + 50, n0 + d - 2) + " a", single(), **LEANC)
        _add("A_text_%d%+d_punct_last" % (n0, d), _prose(n0 + d + 60, n0 + d - 2, True) + "a,", single(minus=True), **LEANC)
for pred_name, pair in (("punct", ",a"), ("blank", " a"), ("letter", "a,")):  # an anchor on a tile's first position
    for n0 in (ANCHOR_TILE, 2 * ANCHOR_TILE):
        body = _prose(n0 + 7, n0 + 300)
        _add("A_tile_first_%s_%d" % (pred_name, n0), body[:n0 - 2] + "b" + pair + "b " + body[n0 + 3:], single(), **LEANC)
for n in (1, ANCHOR_BYTES - 1, ANCHOR_BYTES, ANCHOR_BYTES + 1):  # shorter than a window: StepWin is valid iff wbase + 16 <= n
    _add("A_short_%d" % n, "ab cd,ef g,abc d e f"[:n], single(), **LEANC)
    _add("A_short_word_%d" % n, word(n), single(), n_ids=n, **LEANC)
    _add("A_short_word_fail_%d" % n, word(n, (n - 1,)), single(minus=True), n_ids=1, **LEANC)
for ln in (LEAN_MAX_LEN - 1, LEAN_MAX_LEN, LEAN_MAX_LEN + 1, LEAN_MAX_LEN + 2):  # the lean step: len < 15 || p2 >= end
    for land, tail in (("end_minus_1", "a"), ("end", ""), ("blank_then_end", " "), ("blank_then_word", " ab"), ("punct", ",ab"),
                       ("fail", FAIL + " ab")):
        _add("A_token%d_lands_%s" % (ln, land), "ab " + tok(ln) + tail, pieces(minus=True),
             n_ids=2 + 1 + {"a": 1, "": 0, " ": 0, " ab": 2, ",ab": 3}.get(tail, 0) if land != "fail" else 2 + 1 + 2, **LEANC)
    _add("A_token%d_twice_lands_end" % ln, tok(ln) + tok(ln), pieces(), n_ids=2, **LEANC)

# ---- C: the coverage rule (Linear; soft family) -------------------------------------------------------------------------------------
CLASS_SOFT = dict(lin_anchor_mode=0, lin_staged_emit=0, lin_lean=0, lin_n_wide_words=0, lin_n_long_words=0)
for d in D3:  # a CJK stretch around kMaxAnchorGap: MAX_GAP stays on the class rule
    n = MAX_GAP + d
    _add("C_cjk%+d" % d, "ab." + para(n) + ".ab", soft(), fast=False, longest=n, lin_max_anchor_gap=n, **(COVER if d > 0 else CLASS_SOFT))
_add("C_two_gaps_one_tile", "." + para(2100) + "." + para(2100) + ".ab", soft(), fast=False, longest=2100, **COVER)
_add("C_two_gaps_one_tile_short_second", "." + para(2100) + "." + para(1900) + ".ab", soft(), fast=False, longest=2100, **COVER)
_add("C_gap_starts_on_tile", ("ab." * 700)[:REACH_TILE - 1] + "." + para(2100) + ".ab", soft(), fast=False, longest=2100, **COVER)
_add("C_gap_ends_on_tile", "ab." + para(2 * REACH_TILE - 3) + ".ab", soft(), fast=False, longest=2 * REACH_TILE - 3, **COVER)
_add("C_gap_tile_to_tile", ("ab." * 700)[:REACH_TILE - 1] + "." + para(2 * REACH_TILE) + ".ab", soft(), fast=False,
     longest=2 * REACH_TILE, **COVER)
for crossed, n in ((0, 100), (1, 2500), (3, 6200)):  # behind a paragraph that ends at 2102: tiles end at 4096, 6144, 8192
    head = "." + para(2100) + ". "
    assert (len(head) + 8 + n) // REACH_TILE - (len(head) + 8) // REACH_TILE == crossed
    _add("C_fail_word_crosses_%d" % crossed, head + "ab cd " + FAIL + word(n) + " ab.ab", soft(minus=True), fast=False, **COVER)
    _add("C_fail_word_crosses_%d_to_end" % crossed, head + "ab cd " + FAIL + word(n), soft(minus=True), fast=False, **COVER)
    _add("C_blank_run_crosses_%d" % crossed, head + "ab cd ab" + " " * n + "ab.ab", soft(minus=True), fast=False, **COVER)
    _add("C_blank_run_crosses_%d_to_end" % crossed, head + "ab cd ab" + " " * n, soft(minus=True), fast=False, **COVER)
# leading blanks in front of a first position that is no anchor (the blank is soft): the k == 0 branch of walk_kernel.  The
# gap runs from the text start to the first anchor, the '.' behind the one-letter first word: MAX_GAP - 1 blanks stay on the
# class rule, MAX_GAP blanks make a gap of MAX_GAP + 1 and switch
for lead in (1, ANCHOR_BYTES - 1, ANCHOR_BYTES, MAX_GAP - 1, MAX_GAP, MAX_GAP + 1):
    _add("C_leading_blanks_%d" % lead, " " * lead + "a.ab cd.e", soft(), fast=False, lin_max_anchor_gap=max(lead + 1, 5), n_ids=1 + 1 + 2 + 2 + 1 + 1,
         **(COVER if lead + 1 > MAX_GAP else CLASS_SOFT))
    _add("C_leading_blanks_%d_fail" % lead, " " * lead + "ab" + FAIL + " ab.ab cd.e", soft(minus=True), fast=False, lin_max_anchor_gap=lead + 6,
         n_ids=1 + 2 + 1 + 2 + 2 + 1 + 1, **(COVER if lead + 6 > MAX_GAP else CLASS_SOFT))
# the same first word where a long gap elsewhere switches to the coverage rule: the leading blanks are short of a long gap, so
# the class rule stands there, makes the first word no anchor, and cover_flags_kernel has to flag it
for lead in (1, ANCHOR_BYTES, WAVE, MAX_GAP - 6):
    _add("C_leading_blanks_%d_gap_elsewhere" % lead, " " * lead + "efgab.ab cd." + para(MAX_GAP + 10) + ".ab", soft(), fast=False,
         lin_max_anchor_gap=MAX_GAP + 10, **COVER)
    _add("C_leading_blanks_%d_gap_elsewhere_fail" % lead, " " * lead + "ab" + FAIL + " ab.ab cd." + para(MAX_GAP + 10) + ".ab",
         soft(minus=True), fast=False, **COVER)
# the lean walk under the coverage rule steps over one blank inside its window: a 15-symbol token in front of it
for ln in (LEAN_MAX_LEN - 1, LEAN_MAX_LEN, LEAN_MAX_LEN + 1):
    _add("C_token%d_blank_word_fails" % ln, "." + tok(ln) + " ab" + FAIL + ".ab " + tok(ln) + " ab." + para(MAX_GAP + 10) + ".ab",
         soft(minus=True), fast=False, **COVER)

GROUP_SIZES = {"W": 60, "L": 35, "S": 35, "B": 31, "A": 64, "C": 43}  # asserted by test_walk_cases.py


# ---- F: seeded composition -------------------------------------------------------------------------------------------------------
F_SEEDS = 200
_F_LENGTHS = [1, 3, 4, 5, 14, 15, 16, 17, WIDE_MIN - 1, WIDE_MIN, WIDE_MIN + 1, WAVE - 1, WAVE, WAVE + 1, WIDE_WINDOW - 1, WIDE_WINDOW,
              WIDE_WINDOW + 1, 2 * WIDE_WINDOW - 1, 2 * WIDE_WINDOW, 2 * WIDE_WINDOW + 1, MAX_GAP - 1, MAX_GAP, MAX_GAP + 1, 3000]
_F_BLANKS = [2, ANCHOR_BYTES, WAVE - 1, WAVE, WAVE + 1, 200]
_F_FAMILIES = [("single", single, True), ("minus", lambda: single(minus=True), True), ("pieces", lambda: pieces(minus=True), True),
               ("soft", lambda: soft(minus=True), False), ("no_unk", lambda: single(minus=True, unk=False), True),
               ("cjk", lambda: with_cjk(minus=True), True)]


def _composed(seed):
    rng = random.Random(9000 + seed)
    fam_name, fam, fast = _F_FAMILIES[seed % len(_F_FAMILIES)]
    short = seed % 7 == 3  # stretches of at most kWideMin positions only: the lean walk alone
    parts = []
    if rng.random() < 0.3:
        parts.append(" " * rng.choice(_F_BLANKS))
    for _ in range(rng.randint(3, 12)):
        n = rng.choice(_F_LENGTHS[:9] if short else _F_LENGTHS if rng.random() < 0.8 else _F_LENGTHS[:17])
        r = rng.random()
        if fam_name in ("pieces", "soft") and r < 0.3:
            w = "".join(rng.choice([tok(14), tok(15), tok(16), tok(17), "pq", word(3), word(1)]) for _ in range(n // 8 + 1))[:n]
        elif fam_name == "soft" and r < 0.45:
            w = para(n)
        else:
            w = word(n, [rng.randrange(n)] if rng.random() < 0.15 else (), start=rng.randint(0, 6))
        sep = rng.choice([" ", ",", "."] if short else [" ", " ", ",", CJK[0], " " * rng.choice(_F_BLANKS), ".", ", "])
        parts.append(w + sep)
    if rng.random() < 0.5 and not short:
        parts.append(word(rng.choice(_F_LENGTHS[:20])))
    return "".join(parts), fam(), {}


for _seed in range(F_SEEDS):
    CASES["F_%03d" % _seed] = ((lambda s=_seed: _composed(s)), _F_FAMILIES[_seed % len(_F_FAMILIES)][2])

GROUPS = ("W", "L", "S", "B", "A", "C", "F")


def names(groups="WLSBAC"):
    return [n for n in CASES if n[0] in groups]


def build(name):
    """-> (text bytes, vocab lines, expect): expect["linear"], expect["fast"] (None: not compared) the model's statistics,
    expect["claims"] the builder's"""
    f, fast = CASES[name]
    text, vocab, claims = f()
    m = Model(text, vocab)
    return text.encode("utf-8"), vocab, dict(linear=m.linear(), fast=m.fast() if fast else None, claims=claims, model=m)


# one representative per group, plus the dense and the abutting-lists cases: embedded in a text above kRadixSmallN, and (the
# first two) encoded between the two encodes of every other case on one handle
EMBEDDED = ["W_token_straddles_window", "L_several", "S_tokens+1_fail", "B_anchors_%d+1" % WB_WORDS, "A_token15_lands_blank_then_word",
            "C_cjk+1", "W_dense", "B_punct_%d+1" % WB_WORDS]
