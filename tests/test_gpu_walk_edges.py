"""GPU tests (-m gpu) of the walk at its stretch, window and list edges (csrc/walk.h, csrc/fast.h, linear_path.h::walk,
fast_path.h), on the inputs of walk_cases.py.  Every case of groups W (wide walk), L (long words), S (staging and
rollback), B (dealing and lists), A (anchor tiles and windows) and C (coverage rule):

  - Linear ids equal the CPU oracle on three handles: default, WP_OPT_SPARSE_EMIT=1, WP_OPT_COVER_ANCHORS=1;
  - encode_with_offsets in both units equals offsets_model on the same three handles;
  - where the fast entry point applies, fast_encode equals the oracle's on the default and the sparse handle;
  - on the default handle wp_stats and wp_walk_stats equal what the model of the class rule says the input reaches
    (anchor mode, staged, lean, wide words, long words, gap; the anchor count where the class rule makes the list), for
    Linear and for fast: a case that no longer reaches its branch fails;
  - a second encode on the same handle, with a text of another group in between (a wide word for group L, long words for
    the others), gives the same ids: scalars and scratch are reused.

Group F, 200 seeded compositions of the same edge lengths, is compared the same way without the branch.  All of W to C
run once more in the bounds-checking build with guard zones (a child process), and eight cases — one per group, the dense
wide word and the abutting lists — are embedded in the middle and at the end of a text above kRadixSmallN, where the walk
looks steps up by key and round 0 has dropped the blanks.

Wall time against the rest of the -m gpu suite has not been measured in one job yet (the aim is under a fifth on top; if it is
above, group F is the one to trim first: it is 200 of the 470 cases).

Found by this file: F_021 — soft blanks in front of the first word, and a long gap elsewhere that switches the walk to the
coverage rule.  The class rule still stood around the first word, made it no anchor, and no lane walked it (its ids were
missing).  cover_flags_kernel now flags the text's first non-blank position; the C_leading_blanks_*_gap_elsewhere cases pin it."""
import functools
import json
import os
import traceback

import numpy as np
import pytest

import offsets_model as OM
import oracle_lib as O
import round0_cases as R
import walk_cases as K
import wordpiece_amd as W
from wordpiece_amd import synth

pytestmark = pytest.mark.gpu
PKG = os.path.dirname(os.path.abspath(W.__file__))

LINEAR_FIELDS = ("anchor_mode", "staged_emit", "n_anchors")
WALK_FIELDS = ("lean", "n_wide_words", "n_long_words", "max_anchor_gap")


def _handle(vocab, opt=None):
    gv = W.Vocab(vocab)
    if opt is not None:
        gv.set_option(opt, 1)
    return gv


def _branch(gv):
    st, ws = gv.stats(), gv.walk_stats()
    out = {k: st[k] for k in LINEAR_FIELDS}
    out.update({k: ws[k] for k in WALK_FIELDS})
    return out


def _assert_branch(got, want, label):
    want = {k: v for k, v in want.items() if v is not None}  # (n_anchors under the coverage rule: not modelled)
    assert {k: got[k] for k in want} == want, (label, got, want)


@functools.lru_cache(maxsize=None)
def _between(group):
    """the text encoded between the two encodes of a case: another group's, so that the handle's scratch and scalars
    (the wide count, the long-word list, the per-position array) are left by another variant of the walk"""
    return K.build("W_copy_trip_unlike" if group == "L" else "L_several")[0]


def check_case(name, branch=True, debug_build=False):
    text, vocab, expect = K.build(name)
    ov = O.Vocab(vocab)
    exp = ov.encode(text)
    ids_m, spans, t, starts = OM.encode_spans(text, vocab)
    assert ids_m == exp.tolist(), name
    want_offs = {"char": np.array(spans, dtype=np.int64).reshape(-1, 2),
                 "byte": np.array(OM.to_bytes(spans, text, starts), dtype=np.int64).reshape(-1, 2)}
    exp_fast = ov.fast_encode(text) if expect["fast"] is not None else None
    options = (None,) if debug_build else (None, W.WP_OPT_SPARSE_EMIT, W.WP_OPT_COVER_ANCHORS)
    for opt in options:
        gv = _handle(vocab, opt)
        ids = gv.encode(text)
        got = _branch(gv)
        print(name, "opt", opt, got, flush=True)
        assert np.array_equal(ids, exp), (name, opt, "ids")
        if debug_build:
            assert gv.stats()["reserved0"] == 1 and gv.stats()["guard_zones"] > 0, "not the bounds-checking build with guard zones"
        if opt is None and branch:
            _assert_branch(got, expect["linear"], name + " linear")
        for unit in ("char", "byte"):
            ids_o, offs = gv.encode_with_offsets(text, unit)
            assert np.array_equal(np.array(ids_o), exp), (name, opt, unit, "ids of the offsets call")
            assert np.array_equal(np.array(offs, dtype=np.int64).reshape(-1, 2), want_offs[unit]), (name, opt, unit, "offsets")
        if exp_fast is not None and opt != W.WP_OPT_COVER_ANCHORS:
            assert np.array_equal(gv.fast_encode(text), exp_fast), (name, opt, "fast ids")
            if opt is None and branch:
                _assert_branch(_branch(gv), expect["fast"], name + " fast")
        if opt is None:  # the same handle again, another variant's text in between
            other = _between(name[0])
            assert np.array_equal(gv.encode(text), exp), (name, "second encode")
            assert np.array_equal(gv.encode(other), ov.encode(other)), (name, "text in between")
            assert np.array_equal(gv.encode(text), exp), (name, "encode behind another text")
            if branch:
                _assert_branch(_branch(gv), expect["linear"], name + " linear, third encode")
            if exp_fast is not None:
                assert np.array_equal(gv.fast_encode(other), ov.fast_encode(other)), (name, "fast, text in between")
                assert np.array_equal(gv.fast_encode(text), exp_fast), (name, "fast behind another text")


@pytest.mark.parametrize("name", K.names())
def test_walk_edge(name):
    check_case(name)


@pytest.mark.parametrize("name", K.names("F"))
def test_walk_composed(name):
    check_case(name, branch=False)


# ---- the bounds-checking build with guard zones -------------------------------------------------------------------------------

def _run_debug(out_json):
    """(in a child process on libwordpiece_amd_dbg.so with WP_ARENA_GUARD=1) every case of W to C on the default handle; the
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


def test_walk_edges_bounds_build(tmp_path):
    """Groups W to C in the bounds-checking build with a guard zone behind every arena allocation: a list, a spill or a
    span written one slot too far (the dense word, the abutting lists) makes the encode fail."""
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    out = tmp_path / "results.json"
    r = R.run_in_child(tmp_path, "test_gpu_walk_edges", "_run_debug", (str(out),), {"WP_LIB": dbg, "WP_ARENA_GUARD": "1"},
                       timeout=900, check=False)
    results = {}
    if out.exists():
        with open(str(out)) as f:
            results = json.load(f)
    tail = "child ended with %d: %s %s" % (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    bad = {n: results.get(n, "not run") for n in K.names() if results.get(n) != "ok"}
    assert not bad and r.returncode == 0 and "CHILD_OK" in r.stdout, "\n".join("%s: %s" % kv for kv in sorted(bad.items())[:4]) + tail


# ---- the same inputs inside a text above kRadixSmallN ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _corpus():
    return synth.english_corpus(2_400_000, seed=5, vocab_size=3000)[0]


@pytest.mark.parametrize("name", K.EMBEDDED)
def test_walk_edge_embedded_at_size(name):
    """The case's text in the middle and at the end of 2.4 MB of English words, with the case's vocabulary: the walk runs
    with the key-space lookup and, the blanks being common, without the blank-start suffixes, as the default path at size."""
    case, vocab, _ = K.build(name)
    corpus = _corpus()
    half = corpus.index(b" ", len(corpus) // 2)
    text = corpus[:half] + b" " + case + b" " + corpus[half + 1:] + b" " + case
    gv = W.Vocab(vocab)
    ids = gv.encode(text)
    st = gv.stats()
    print(name, {k: st[k] for k in ("n_total", "round0_keys_only", "round0_sorted", "hist_in_keys", "anchor_mode", "staged_emit")},
          gv.walk_stats(), flush=True)
    assert st["n_total"] > R.RADIX_SMALL_N and st["round0_keys_only"] == 1 and st["round0_sorted"] < st["n_total"], st
    assert np.array_equal(ids, O.Vocab(vocab).encode(text, threads=8)), name
