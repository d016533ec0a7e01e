"""GPU tests (-m gpu) of the refinement of the needed groups along the token trie — csrc/prune.h (need_groups, needed_fill),
csrc/trie.h, csrc/local_sort.h, linear_path.h::trie_round_finish and the group starts of csrc/scanline.h — on the inputs of
refine_cases.py.  Every named case of groups G (small groups, LDS windows), L (large groups), T (trie descent), D (the shared
stretch of a group), R (tokens against each other), P (position in slot space), N (node counts) and Y (wide symbols):

  - the default handle, WP_OPT_SORT_BLANKS and WP_OPT_INDEXED_ROUND0 give the oracle's ids;
  - wp_refine_stats and the named wp_stats fields of the default handle equal what the construction says: a case that no
    longer reaches its branch fails;
  - on a WP_OPT_KEEP_DEBUG handle (full rank table, the trie round beside the rank store, key_lookup 0) the two best arrays,
    taken through the rank array, equal refine_cases.longest_matches at every text position, and the suffix array
    restricted to every needed group is a permutation of the group's members;
  - WP_OPT_VOCAB_IN_S gives the same ids for groups G, L, R and P (the same segmented sort and large-group path, driven by
    the doubling rounds); not for N, whose 2^18-symbol vocabularies would sit in S, nor for T, D, Y, which the issue leaves out;
  - encode_with_offsets (code points) equals offsets_model on the default handle;
  - the same handle again, with a text of another population in between (refine_cases.between_text): same ids, same statistics.

Group F (100 seeded compositions) gets the same checks without the expected statistics.  All named cases run once more in
the bounds-checking build with guard zones (a child process); one case each of G, L, T and P is embedded in the middle and
at the end of 2.4 MB of English words, and one L case in a text above 2^22 symbols on a WP_OPT_KEEP_DEBUG handle (the rank
store by LDS windows, the trie round beside it).

Wall time (measured on an MI355X, in one job with the first half of the rest of the -m gpu suite): 52 s for the 208 tests of
this file, 872 s for the 985 other GPU tests (388 s + 484 s, two jobs): 6 % on top.  Group F takes a quarter of it and is
the first to trim.

Found by this file: no wrong id.  Against two deliberately wrong scratch builds — trie_token_range_kernel's second search
one node short; the one-byte branch of trie_chain_match rounded down to whole 8-symbol loads — 99 and 94 of the 106 named
and embedded tests fail (23 / 24 cases of T and 14 / 14 of R among them); the wide-symbol cases of Y pass the second, as they
must: they take the generic loop."""
import functools
import json
import os
import traceback

import numpy as np
import pytest

import offsets_model as OM
import oracle_lib as O
import refine_cases as K
import round0_cases as R
import wordpiece_amd as W
from wordpiece_amd import synth

pytestmark = pytest.mark.gpu
PKG = os.path.dirname(os.path.abspath(W.__file__))
STATS_FIELDS = ("trie_refine", "round0_keys_only", "needed_after_round0", "rounds", "n_total")


@functools.lru_cache(maxsize=4)
def reference(name):
    """computed once per case and left unchanged: the oracle's ids, the model's spans, longest matches and group members"""
    c = K.build(name)
    exp = O.Vocab(c.vocab).encode(c.text)
    ids_m, spans, _, _ = OM.encode_spans(c.text, c.vocab)
    assert ids_m == exp.tolist(), name
    want_p, want_s = K.longest_matches(c.text, c.vocab)
    groups = [v for v in K.group_populations(c.text, c.vocab).values() if len(v) >= 2]
    return dict(ids=exp, spans=np.array(spans, dtype=np.int64).reshape(-1, 2), best_p=np.array(want_p, dtype=np.int32),
                best_s=np.array(want_s, dtype=np.int32), groups=groups)


def _handle(vocab, opt=None):
    gv = W.Vocab(vocab)
    if opt is not None:
        gv.set_option(opt, 1)
    return gv


def _branch(gv):
    st = gv.stats()
    return gv.refine_stats(), {k: st[k] for k in STATS_FIELDS}


def check_case(name, branch=True, debug_build=False):
    c = K.build(name)
    ref = reference(name)
    exp = ref["ids"]
    want = K.expected_stats(c)
    gv = _handle(c.vocab)
    ids = gv.encode(c.text)
    got = _branch(gv)
    print(name, got, flush=True)
    assert np.array_equal(ids, exp), (name, "ids")
    if branch:
        assert got == want, (name, got, want)
    if debug_build:
        st = gv.stats()
        assert st["reserved0"] == 1 and st["guard_zones"] > 0, "not the bounds-checking build with guard zones"
        return
    for opt in (W.WP_OPT_SORT_BLANKS, W.WP_OPT_INDEXED_ROUND0):
        assert np.array_equal(_handle(c.vocab, opt).encode(c.text), exp), (name, opt, "ids")
    if name[0] in K.VOCAB_IN_S_GROUPS:
        assert np.array_equal(_handle(c.vocab, W.WP_OPT_VOCAB_IN_S).encode(c.text), exp), (name, "ids, vocabulary in S")
    # the debug views of the default layout
    dv = _handle(c.vocab, W.WP_OPT_KEEP_DEBUG)
    assert np.array_equal(dv.encode(c.text), exp), (name, "ids, debug handle")
    rs = dv.refine_stats()
    assert rs["key_lookup"] == 0 and dv.stats()["trie_refine"] == 1, (name, rs)
    if branch:
        assert {k: v for k, v in rs.items() if k != "key_lookup"} == {k: v for k, v in want[0].items() if k != "key_lookup"}, (name, rs)
    n = want[1]["n_total"]
    rank = dv.debug_fetch(2, n)[:n - 1]
    assert np.array_equal(dv.debug_fetch(4, n)[rank], ref["best_p"]), (name, "longest prefix-class token by position")
    assert np.array_equal(dv.debug_fetch(5, n)[rank], ref["best_s"]), (name, "longest ##-class token by position")
    sa = dv.debug_fetch(1, n)
    for members in ref["groups"]:  # (members that end in one trie node stay tied: they share the rank of their first slot)
        r = rank[members]
        lo, k = int(r.min()), len(members)
        assert int(r.max()) < lo + k and np.array_equal(np.sort(sa[lo:lo + k]), np.array(members)), \
            (name, "the group's slots hold its members", members[:4], lo, int(r.max()))
    # offsets, and the handle's state
    ids_o, offs = gv.encode_with_offsets(c.text, "char")
    assert np.array_equal(np.array(ids_o), exp), (name, "ids of the offsets call")
    assert np.array_equal(np.array(offs, dtype=np.int64).reshape(-1, 2), ref["spans"]), (name, "offsets")
    other = K.between_text(c)
    assert np.array_equal(gv.encode(other), O.Vocab(c.vocab).encode(other)), (name, "text in between")
    assert np.array_equal(gv.encode(c.text), exp), (name, "encode behind another text")
    if branch:
        assert _branch(gv) == want, (name, "statistics behind another text", _branch(gv), want)


@pytest.mark.parametrize("name", K.names())
def test_refine_edge(name):
    check_case(name)


@pytest.mark.parametrize("name", K.names("F"))
def test_refine_composed(name):
    check_case(name, branch=False)


# ---- the bounds-checking build with guard zones -------------------------------------------------------------------------------

def _run_debug(out_json):
    """(in a child process on libwordpiece_amd_dbg.so with WP_ARENA_GUARD=1) every named case on the default handle; the
    outcome of each goes to out_json as it comes.  An error that is no failed comparison ends the run: nothing is started
    on the GPU behind it."""
    results = {}
    for name in K.names():
        stop = False
        try:
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


def test_refine_edges_bounds_build(tmp_path):
    """Every named case in the bounds-checking build (the candidate runs, the list's slots and the key-space steps are
    range-checked: kSiteCandRun, kSiteListSlot, kSiteKeyStep) with a guard zone behind every arena allocation."""
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    out = tmp_path / "results.json"
    r = R.run_in_child(tmp_path, "test_gpu_refine_edges", "_run_debug", (str(out),), {"WP_LIB": dbg, "WP_ARENA_GUARD": "1"},
                       timeout=900, check=False)
    results = {}
    if out.exists():
        with open(str(out)) as f:
            results = json.load(f)
    tail = "child ended with %d: %s %s" % (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    bad = {n: results.get(n, "not run") for n in K.names() if results.get(n) != "ok"}
    assert not bad and r.returncode == 0 and "CHILD_OK" in r.stdout, "\n".join("%s: %s" % kv for kv in sorted(bad.items())[:4]) + tail


# ---- the same inputs inside texts above kRadixSmallN and above 2^22 symbols -------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _corpus():
    return synth.english_corpus(2_400_000, seed=5, vocab_size=3000)[0]


@pytest.mark.parametrize("name", K.EMBEDDED)
def test_refine_edge_embedded_at_size(name):
    """The case's text in the middle and at the end of 2.4 MB of English words, with the case's vocabulary: full-size radix
    tiles, the key builder's histogram, the blank-start suffixes left out.  The first half of the case's words stands in the
    middle and the second half at the end, so every group keeps its size and the text ends where the case ends."""
    c = K.build(name)
    corpus = _corpus()
    half = corpus.index(b" ", len(corpus) // 2)
    cut = c.text.index(b" ", len(c.text) // 2)
    text = corpus[:half] + b" " + c.text[:cut] + b" " + corpus[half + 1:] + c.text[cut:]
    gv = W.Vocab(c.vocab)
    ids = gv.encode(text)
    st, rs = gv.stats(), gv.refine_stats()
    print(name, {k: st[k] for k in ("n_total", "round0_keys_only", "round0_sorted", "hist_in_keys")}, rs, flush=True)
    assert st["n_total"] > R.RADIX_SMALL_N and st["hist_in_keys"] == 1 and st["round0_sorted"] < st["n_total"], st
    want = K.expected_stats(c)[0]
    assert rs["n_groups"] == want["n_groups"] and rs["n_entries"] == want["n_entries"] and rs["trie_nodes"] == want["trie_nodes"], rs
    assert rs["n_large_groups"] == want["n_large_groups"] and rs["n_large_entries"] == want["n_large_entries"], rs
    assert np.array_equal(ids, O.Vocab(c.vocab).encode(text, threads=8)), name


def test_refine_large_groups_beside_window_store():
    """An L case in a text of at least 2^22 symbols on a WP_OPT_KEEP_DEBUG handle: the rank store assembles LDS windows and
    the trie round starts beside it (store_ranks_round0).  Ids only."""
    c = K.build("L_three_large")
    corpus = _corpus()
    text = corpus + b" " + c.text + b" " + corpus
    gv = _handle(c.vocab, W.WP_OPT_KEEP_DEBUG)
    ids = gv.encode(text)
    st, rs = gv.stats(), gv.refine_stats()
    print(st["n_total"], rs, flush=True)
    assert st["n_total"] >= R.WINDOW_STORE_N and rs["key_lookup"] == 0 and rs["n_large_groups"] == 3, (st["n_total"], rs)
    assert np.array_equal(ids, O.Vocab(c.vocab).encode(text, threads=8))
