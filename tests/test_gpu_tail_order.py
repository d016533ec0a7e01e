"""GPU tests (-m gpu) of the stretch between the last round-0 pass and the walk as linear_path.h queues it now
(scanlines / side_tables / fill_tables / walk; csrc/scanline.h: mark_cover_totals_kernel, mark_cover_kernel,
step_tables_kernel, key_starts_kernel, key_steps_flag_kernel; linear_path.h: token_marks_kernel):

  cover scan, one workgroup per chunk    M = 1, C - 1, C, C + 1, 2 C + 1 marks (C = kCoverThreads * kCoverItems), both classes
                                         interleaved.  The covering word "b" is a token of one class only and mark 0, the last
                                         mark is "bzz" in the other class only: where "bzzz" starts, at a word's start and
                                         inside a word, the longest token of the first class is "b", found from the last mark
                                         on, so a lost carry shows in the step views of every case of more than one chunk;
                                         once per class of the covering token
  keys-only sort of the step starts      P = 4 M + 1 on both sides of the small sort's tile of 1024 keys (M = 255, 256) times
                                         n_total = 2^16 - 1, 2^16, 2^16 + 1 (the third pass of 8 bits appears); rows of tokens
                                         that never occur (equal starts); starts that differ in the lowest and in the highest
                                         digit only are the marks of "b..." and the marks of "z"
  fused tables                           packed == 0 through one token of kStepMaxLen symbols; a needed group present (two
                                         families, 2 and 65 members: steps on a group's first slot and behind its last) and
                                         absent; M = 1 and M = 0 (no trie, no key lookup: the old order, asserted through
                                         wp_step_stats); equal and unequal index shifts with three or four tables in one launch:
                                         K_shift_all_16383 / _16384 of step_cases.py, here also in the bounds child
  ranks of the needed groups             a needed-group case on the default and on a WP_OPT_KEEP_DEBUG = 2 handle (the step
                                         views read the ranks); a periodic text with more than 2^22 list entries, whose
                                         expected ids are one period's oracle ids repeated
  anchor scalars by event                five unlike texts back to back through one handle, default / WP_OPT_COVER_ANCHORS /
                                         WP_OPT_SPARSE_EMIT, and three shards of unlike sizes through encode_stream

Expected ids: oracle_lib.  Expected longest matches: step_cases.longest_matches through views 8-11 of a WP_OPT_KEEP_DEBUG = 2
handle.  Every reference is computed once and left unchanged.  All named cases run once more in a child process on the
bounds-checking build with guard zones.

Proof that the file can fail — two scratch builds, never committed, value-only mutations, run on an MI355X against the 30
tests of this file:
  (a) the carry between cover chunks dropped (mark_cover_kernel ignores the chunk totals): 6 fail — the four cover cases of
      more than one chunk (M = C + 1 and 2 C + 1, both classes) and K_shift_all_16383 / _16384 (two chunks).  The
      cover cases of M = 1, C - 1 and C have a single chunk and nothing to carry; the bounds child loads
      libwordpiece_amd_dbg.so by its path, not the scratch build.
  (b) step_tables_kernel writing the slot-space value where kStepNeeded belongs: 5 fail — every named case with a needed
      group (tables_unpacked, tables_groups, ranks_three_large, K_shift_all_16383 / _16384).  The periodic text of 2^22
      entries passes under (b), as do the cases without a needed group."""
import functools
import json
import os
import random
import traceback

import numpy as np
import pytest

import oracle_lib as O
import refine_cases as RC
import round0_cases as R
import step_cases as K
import wordpiece_amd as W

pytestmark = pytest.mark.gpu
PKG = os.path.dirname(os.path.abspath(W.__file__))
C = K.COVER_CHUNK


class Case:
    def __init__(self, name, text, vocab):
        self.name, self.text, self.vocab = name, text, list(vocab)
        self.n_text = len(text.decode("utf-8"))


def cover_case(M, cls):
    """M eligible lines.  The covering word "b" is a token of class `cls` alone ("" or "##") and mark 0; the last mark is "bzz"
    in the OTHER class alone (M >= 2); every other line sorts between the two.  At a position where "bzzz" starts, the longest
    token of class `cls` is therefore "b": the lookup starts at the last mark and needs the cover carried through every chunk."""
    other = "" if cls else "##"
    tail = [other + "bzz"] if M >= 2 else []
    body = [w for w in K._marks_vocab(M + 2) if K.word_of(w) != "b"][:M - 1 - len(tail)]
    lines = [cls + "b"] + body + tail
    assert len(lines) == M and len(set(lines)) == M
    ws = sorted({K.word_of(w) for w in lines})
    rng = random.Random(M)
    words = [rng.choice(ws) for _ in range(1200)] + [rng.choice(ws) + rng.choice(ws) for _ in range(600)]
    words += ["bzzz"] * 9 + ["gbzzz"] * 9 + ["bz"] * 3 + ["b"] * 5 + ws[-3:] * 3   # ("gbzzz": the same start inside a word)
    rng.shuffle(words)
    return Case("cover_%d_%s" % (M, "suffix" if cls else "prefix"), " ".join(words).encode(), ["[UNK]"] + lines)


def sort_case(M, n_total):
    """M lines, a third of which occur in the text (the others: rows of equal starts), a text of n_total - 1 code points"""
    lines = K._marks_vocab(M - 2) + ["z", "##z"]
    ws = sorted({K.word_of(w) for w in lines})
    text = K._exact_text(random.Random(n_total + M), ws[::3] + ["bz", "zb"], n_total - 1)
    return Case("sort_%d_%d" % (M, n_total), text.encode(), ["[UNK]"] + lines)


def table_case(kind):
    lines = K._marks_vocab(20)
    ws = sorted({K.word_of(w) for w in lines})
    rng = random.Random(len(kind))
    words = [rng.choice(ws) for _ in range(300)] + [rng.choice(ws) + rng.choice(ws) for _ in range(100)] + ["bz"] * 4
    extra = []
    if kind == "unpacked":        # one token of kStepMaxLen symbols: step values carry no length
        extra = ["g" * K.STEP_MAX_LEN]
        words += ["g" * K.STEP_MAX_LEN, "g" * 40]
    elif kind == "groups":        # two needed groups: steps on a group's first slot and on the slot behind its last
        fams = [RC.Family("T", at=[RC.BASE + 1, RC.BASE + 4], k=65), RC.Family("V", at=[RC.BASE + 2], k=2)]
        used = sorted(set("".join(m for f in fams for m in f.members)))
        extra = [ch for ch in used if ch not in lines] + ["##" + ch for ch in used] + [t for f in fams for t in f.tokens]
        words += [m for f in fams for m in f.members]
    elif kind == "one_mark":
        lines = ["b"]
    elif kind == "no_mark":       # M = 0: no trie, no key lookup — the stage keeps its old order on the main stream
        lines = []
    rng.shuffle(words)
    return Case("tables_" + kind, " ".join(words).encode(), ["[UNK]"] + lines + extra)


def rank_case():
    """refine_cases.L_three_large: needed groups on both sides of the LDS sort's largest group, one through the radix path"""
    c = RC.build("L_three_large")
    return Case("ranks_three_large", c.text, c.vocab)


CASES = {}
for _M in (1, C - 1, C, C + 1, 2 * C + 1):
    for _cls in ("", "##"):
        CASES["cover_%d_%s" % (_M, "suffix" if _cls else "prefix")] = functools.partial(cover_case, _M, _cls)
for _M in (255, 256):
    for _n in ((1 << 16) - 1, 1 << 16, (1 << 16) + 1):
        CASES["sort_%d_%d" % (_M, _n)] = functools.partial(sort_case, _M, _n)
for _kind in ("plain", "unpacked", "groups", "one_mark", "no_mark"):
    CASES["tables_" + _kind] = functools.partial(table_case, _kind)
# bit_length(4 P) on both sides of kStepBucketBits in a text above 2^19 symbols: three or four tables in one launch
for _name in ("K_shift_all_16383", "K_shift_all_16384"):
    CASES[_name] = functools.partial(K.build, _name)
CASES["ranks_three_large"] = rank_case
NAMED = list(CASES)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the case, the oracle's ids, the model's longest matches and their lengths: computed once"""
    c = CASES[name]()
    exp = O.Vocab(c.vocab).encode(c.text, threads=8)
    want_p, want_s = K.longest_matches(c.text, c.vocab)
    lens = np.array([len(K.word_of(w)) for w in c.vocab] + [0], dtype=np.int32)
    best_p, best_s = np.array(want_p, dtype=np.int32), np.array(want_s, dtype=np.int32)
    nonblank = np.array([ch != " " for ch in c.text.decode("utf-8")])
    return c, exp, dict(best_p=best_p, best_s=best_s, len_p=lens[best_p], len_s=lens[best_s], nonblank=nonblank)


def check_views(c, ref, gv):
    v = [gv.debug_fetch(w, c.n_text) for w in (8, 9, 10, 11)]
    nb = ref["nonblank"]
    assert (v[0][~nb] == -1).all() and (v[1][~nb] == -1).all(), (c.name, "blanks")
    assert np.array_equal(v[0][nb], ref["best_p"][nb]), (c.name, "longest prefix-class token by position")
    assert np.array_equal(v[1][nb], ref["best_s"][nb]), (c.name, "longest ##-class token by position")
    assert np.array_equal(v[2][nb], ref["len_p"][nb]) and np.array_equal(v[3][nb], ref["len_s"][nb]), (c.name, "lengths")


def check_case(name, debug_build=False):
    c, exp, ref = reference(name)
    gv = W.Vocab(c.vocab)
    ids = gv.encode(c.text)
    ss, rs = gv.step_stats(), gv.refine_stats()
    print(name, ss, rs["n_groups"], rs["n_entries"], flush=True)
    assert np.array_equal(ids, exp), (name, "ids")
    assert ss == K.expected_step_stats(c, False, rs["n_groups"]), (name, ss)
    no_mark = name == "tables_no_mark"
    assert ss["key_lookup"] == (0 if no_mark else 1) and gv.refine_sched()["early"] == (0 if no_mark else 1), (name, ss)
    assert ss["n_marks"] == (0 if no_mark else len(K.eligible(c.vocab))), (name, ss)
    if name.startswith("K_shift_all"):
        differ = int(name.endswith("16384"))
        assert (ss["bucket_shift_all"] != ss["bucket_shift"]) == bool(differ) == (ss["key_shift_all"] != ss["key_shift"]), (name, ss)
    if name == "tables_unpacked":
        assert ss["packed"] == 0, ss
    if name == "tables_groups":
        assert rs["n_groups"] >= 2, rs
    if name == "ranks_three_large":
        assert rs["n_groups"] >= 3 and rs["n_large_groups"] >= 1, rs
    if debug_build:
        st = gv.stats()
        assert st["reserved0"] == 1 and st["guard_zones"] > 0, "not the bounds-checking build with guard zones"
    pv = W.Vocab(c.vocab)
    pv.set_option(W.WP_OPT_KEEP_DEBUG, 2)
    assert np.array_equal(pv.encode(c.text), exp), (name, "ids, step-view handle")
    check_views(c, ref, pv)
    if debug_build:
        return
    late = W.Vocab(c.vocab)
    late.set_option(W.WP_OPT_LATE_REFINE, 1)
    assert np.array_equal(late.encode(c.text), exp), (name, "ids, late refinement")
    assert dict(late.step_stats(), n_steps=0) == dict(ss, n_steps=0), (name, late.step_stats())


@pytest.mark.parametrize("name", NAMED)
def test_tail_case(name):
    check_case(name)


# ---- a list of more than 2^22 entries: the partitioned rank store ---------------------------------------------------------------

def test_ranks_of_a_list_above_2_22_entries():
    """One word of 81 symbols repeated: every suffix shares its key with the long tokens, the list holds nearly every
    position.  The expected ids are one period's oracle ids repeated — no suffix array of the whole text on the host."""
    word = b"ab" * 40 + b"c"
    vocab = ["[UNK]"] + ["ab" * k for k in (1, 2, 5, 9, 14, 20, 33, 40)] + ["##" + "ab" * k for k in (1, 3, 7, 12, 21)] + \
            ["##c", "##b", "##a", "a", "b"]
    reps = (1 << 22) // 33 + 2000   # (33 list entries per word: the suffixes that share the long tokens' key)
    text = b" ".join([word] * reps)
    period = O.Vocab(vocab).encode(word)
    gv = W.Vocab(vocab)
    ids = gv.encode(text)
    rs = gv.refine_stats()
    print(rs, gv.stats()["list_retries"], flush=True)
    assert rs["n_entries"] >= 1 << 22 and gv.refine_sched()["early"] == 1, rs
    assert len(ids) == reps * len(period) and np.array_equal(ids.reshape(reps, len(period)), np.tile(period, (reps, 1)))


# ---- the anchor scalars reach the host by their own copy ------------------------------------------------------------------------

def _sequence():
    lines = K._marks_vocab(64) + ["z", "##z"]
    ws = sorted({K.word_of(w) for w in lines})
    rng = random.Random(3)
    first = [rng.choice(ws) for _ in range(5000)]
    long_word = "".join(rng.choice(ws) for _ in range(K.MAX_ANCHOR_GAP))       # more than kMaxAnchorGap positions
    assert len(long_word) > K.MAX_ANCHOR_GAP
    with_long = [rng.choice(ws) for _ in range(700)] + [long_word] + [rng.choice(ws) for _ in range(300)]
    other = [rng.choice(ws) + "z" for _ in range(1777)]
    texts = [" ".join(first), " ".join(with_long), " " * 3000, " ".join(other), " ".join(first)]
    anchors = [len(first), len(with_long), 0, len(other), len(first)]
    return ["[UNK]"] + lines, [t.encode() for t in texts], anchors


@functools.lru_cache(maxsize=None)
def sequence_reference():
    vocab, texts, anchors = _sequence()
    ov = O.Vocab(vocab)
    return vocab, texts, anchors, [ov.encode(t) for t in texts]


def check_sequence(opt=None):
    vocab, texts, anchors, exp = sequence_reference()
    gv = W.Vocab(vocab)
    if opt is not None:
        gv.set_option(opt, 1)
    for i, t in enumerate(texts):
        ids = gv.encode(t)
        st, ws = gv.stats(), gv.walk_stats()
        print(opt, i, st["n_anchors"], ws, flush=True)
        assert np.array_equal(ids, exp[i]), (opt, i, "ids")
        if opt != W.WP_OPT_COVER_ANCHORS:   # (the coverage rule makes its own anchors inside the words)
            assert st["n_anchors"] == anchors[i], (opt, i, st["n_anchors"], anchors[i])
        else:
            assert st["n_anchors"] >= anchors[i], (opt, i, st["n_anchors"], anchors[i])
        if i == 1 and opt is None:
            assert ws["n_long_words"] == 1 and ws["max_anchor_gap"] > K.MAX_ANCHOR_GAP, ws


@pytest.mark.parametrize("opt", [None, "WP_OPT_COVER_ANCHORS", "WP_OPT_SPARSE_EMIT"])
def test_unlike_texts_back_to_back(opt):
    check_sequence(getattr(W, opt) if opt else None)


def test_three_shards_through_encode_stream():
    vocab, texts, _, exp = sequence_reference()
    order = [0, 1, 3]   # 5000 words, a long word among 1000, 1777 words
    got = {}
    W.Vocab(vocab).encode_stream([texts[i] for i in order], lambda k, ids: got.__setitem__(k, np.array(ids)))
    assert sorted(got) == [0, 1, 2]
    for k, i in enumerate(order):
        assert np.array_equal(got[k], exp[i]), (k, "ids of the shard")


# ---- the bounds-checking build with guard zones ---------------------------------------------------------------------------------

def _run_debug(out_json):
    """(child on libwordpiece_amd_dbg.so with WP_ARENA_GUARD=1) every named case and the sequence; the outcome of each goes to
    out_json as it comes.  An error that is no failed comparison ends the run: nothing is started on the GPU behind it."""
    results = {}
    for name in NAMED + ["sequence"]:
        stop = False
        try:
            if name == "sequence":
                check_sequence()
            else:
                check_case(name, debug_build=True)
            results[name] = "ok"
        except AssertionError:
            results[name] = traceback.format_exc()[-2000:]
        except Exception:
            results[name] = traceback.format_exc()[-2000:]
            stop = True
        with open(out_json, "w") as f:
            json.dump(results, f)
        if stop:
            return


def test_tail_order_bounds_build(tmp_path):
    """kSiteKeyStep (key_steps_check_kernel behind step_tables_kernel), kSiteListSlot, kSiteRankStore, kSiteTokenId and the
    guard zone behind every arena allocation (the chunk totals, the flags of the needed groups) on the new order."""
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    out = tmp_path / "results.json"
    r = R.run_in_child(tmp_path, "test_gpu_tail_order", "_run_debug", (str(out),), {"WP_LIB": dbg, "WP_ARENA_GUARD": "1"},
                       timeout=900, check=False)
    results = {}
    if out.exists():
        with open(str(out)) as f:
            results = json.load(f)
    tail = "child ended with %d: %s %s" % (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    bad = {n: results.get(n, "not run") for n in NAMED + ["sequence"] if results.get(n) != "ok"}
    assert not bad and r.returncode == 0 and "CHILD_OK" in r.stdout, "\n".join("%s: %s" % kv for kv in sorted(bad.items())[:4]) + tail
