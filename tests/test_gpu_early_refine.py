"""GPU tests (-m gpu) of the early refinement of the keys-only round 0 (linear_path.h::refine_early; csrc/prune.h,
need_groups_early_kernel / need_ranges_kernel; csrc/trie.h, trie_token_range_in_list as linear_path.h::token_marks_kernel
calls it; csrc/suffix_array.h,
scatter_list_ranks_kernel): the needed groups are built from the runs of the sorted candidate list and refined in list
space beside the radix passes; only the searches in the sorted keys and the rank scatter wait for the sort.

The named cases of refine_cases.py that reach each branch of the split —

  a group of exactly 2                                    G_group_2
  a singleton (match / before / behind), an absent key    R_once_match _before _behind, R_never_occurs, R_all_once
  several long tokens that share one key (one claim)      R_every_prefix_70, R_inword_family, T_text_end_3
  a long key that is also the range start of a short token  R_every_prefix_70 (every prefix of the stem is a token)
  groups of 2047 / 2048 / 2049 entries, one through the radix path  G_window_4095, G_group_max, L_group_max+1,
                                                          L_group_5000, L_three_large
  a group with the first kept slot / the last             P_smallest, P_largest, P_both

— each embedded in filler of lower-case words just above RADIX_SMALL_N symbols (the smallest size at which the key builder
takes the sort's histogram): ids of the default handle, WP_OPT_LATE_REFINE=1 and WP_OPT_INDEXED_ROUND0=1 against the oracle,
wp_refine_sched.early 1 / 0 / 0, wp_refine_stats equal between the first two and equal to the construction.  The oracle's
ids of a text are computed once and shared.  Further: a blank share on each side of 1/16 (child process without the context
pool: the blank drop on and off), the list overflow and its retry, a list of more than 2^22 entries (the partitioned rank
store), 8 unlike texts through one handle, byte offsets from the device entry point, and all of it once more in the bounds-checking build with guard zones (kSiteCandRun counts a candidate
run that is not the key's equal range in the sorted keys).

Proof that the file can fail — two scratch builds, never committed, run on an MI355X against the 23 tests of this file:
  - gfirst - ghead left out of the ranks alone (scatter_list_ranks_kernel, list_rank_base_kernel): 21 fail.  The two that
    pass have to: R_all_once puts nothing on the list, so no rank is stored, and test_early_refine_bounds_build loads
    libwordpiece_amd_dbg.so by its path, not the scratch build.
  - the base left out of the ranks AND of trie_token_range_list_kernel (the kernel that called trie_token_range_in_list
    then; token_marks_kernel does now): 19 fail.  Besides those two, R_inword_family and
    the 2^22-entry list pass: ranks and token ranges are then both in list space and agree with each other, and the ids
    are right wherever the list positions of a group collide with no other step of the slot-space table.  The first
    build is the sharper one."""
import functools
import json
import os
import random
import traceback

import numpy as np
import pytest

import oracle_lib as O
import refine_cases as K
import round0_cases as R
import wordpiece_amd as W

pytestmark = pytest.mark.gpu
PKG = os.path.dirname(os.path.abspath(W.__file__))

NAMED = ["G_group_2", "R_once_match", "R_once_before", "R_once_behind", "R_never_occurs", "R_all_once", "R_every_prefix_70",
         "R_inword_family", "T_text_end_3", "G_window_4095", "G_group_max", "L_group_max+1", "L_group_5000", "L_three_large",
         "P_smallest", "P_largest", "P_both"]
SPARSE = ["G_group_2", "R_once_before", "L_group_max+1", "P_both"]  # once more in filler with few blanks (no blank drop)
FILL_LETTERS = "ijklmnopqrstuvw"  # no head, body or leave symbol of a family: the filler adds no member to any group
FILL_LEN = R.RADIX_SMALL_N + 100


@functools.lru_cache(maxsize=None)
def filler(dense):
    """lower-case words, one character in 8 a blank (dense: the blank drop is on) or one in 32 (off: words glued)"""
    rng = random.Random(11)
    words = ["".join(rng.choice(FILL_LETTERS) for _ in range(rng.randint(2, 11))) for _ in range(500)]
    return R.sized_text(12 if dense else 13, words, FILL_LEN, FILL_LEN // (8 if dense else 32), blanks=" ", end="letter")


def vocab_of(case):
    singles = [c for c in FILL_LETTERS] + ["##" + c for c in FILL_LETTERS]
    return case.vocab + [t for t in singles if t not in set(case.vocab)]


def embed(case, dense=True):
    """the first half of the case's words in the middle of the filler and the second half at its end: every group keeps its
    size and the text ends where the case ends (refine_cases.EMBEDDED, at the smallest size)"""
    fill = filler(dense)
    half = fill.index(b" ", len(fill) // 2)
    cut = case.text.index(b" ", len(case.text) // 2)
    return fill[:half] + b" " + case.text[:cut] + b" " + fill[half + 1:] + case.text[cut:]


@functools.lru_cache(maxsize=None)
def reference(name, dense=True):
    """(text, vocabulary, oracle ids): computed once per case and left unchanged"""
    c = K.build(name)
    text, vocab = embed(c, dense), vocab_of(c)
    return text, vocab, O.Vocab(vocab).encode(text, threads=8)


def expected_refine(case):
    sizes = [f.k for f in case.families if f.listed]
    large = [s for s in sizes if s > K.LS_MAXGROUP]
    return dict(n_groups=len(sizes), n_entries=sum(sizes), n_large_groups=len(large), n_large_entries=sum(large))


def _handle(vocab, opt=None):
    gv = W.Vocab(vocab)
    if opt is not None:
        gv.set_option(opt, 1)
    return gv


def check_case(name, dense=True, drop=None, debug_build=False):
    """ids three ways, the placement each handle reports, the statistics of both placements.  drop: True / False — the
    blank drop must be on / off (only where the handle's symbol code is its own: a child without the context pool)"""
    c = K.build(name)
    text, vocab, exp = reference(name, dense)
    dv = _handle(vocab)
    ids = dv.encode(text)
    st, rs, sched = dv.stats(), dv.refine_stats(), dv.refine_sched()
    print(name, dense, {k: st[k] for k in ("n_total", "round0_sorted", "round0_candidates", "list_retries")}, rs, sched, flush=True)
    assert np.array_equal(ids, exp), (name, "ids, early refinement")
    assert st["n_total"] > R.RADIX_SMALL_N and st["round0_keys_only"] == 1 and st["hist_in_keys"] == 1, (name, st)
    assert sched["early"] == 1, (name, sched)
    want = expected_refine(c)
    assert {k: rs[k] for k in want} == want, (name, rs, want)
    assert st["needed_after_round0"] == want["n_entries"] and st["rounds"] == (2 if want["n_entries"] else 1), (name, st)
    assert st["round0_candidates"] >= st["needed_after_round0"], (name, st)
    assert st["radix_pass_elems"] == st["n_total"] + 3 * st["round0_sorted"], (name, st)
    if drop is not None:
        assert (st["round0_sorted"] < st["n_total"]) == drop, (name, "blank drop", st["round0_sorted"], st["n_total"])
        if drop:
            assert st["round0_sorted"] == R.kept(text), (name, st["round0_sorted"])
    if debug_build:
        assert st["reserved0"] == 1 and st["guard_zones"] > 0, "not the bounds-checking build with guard zones"
    lv = _handle(vocab, W.WP_OPT_LATE_REFINE)
    assert np.array_equal(lv.encode(text), exp), (name, "ids, late refinement")
    assert lv.refine_sched()["early"] == 0 and lv.stats()["round0_keys_only"] == 1, (name, lv.refine_sched())
    assert lv.refine_stats() == rs, (name, "wp_refine_stats of the two placements", lv.refine_stats(), rs)
    iv = _handle(vocab, W.WP_OPT_INDEXED_ROUND0)
    assert np.array_equal(iv.encode(text), exp), (name, "ids, indexed round 0")
    assert iv.refine_sched()["early"] == 0 and iv.stats()["round0_keys_only"] == 0, (name, iv.refine_sched())


@pytest.mark.parametrize("name", NAMED)
def test_early_refine_case(name):
    check_case(name)


def _run_blank_shares(out_json):
    """(child without the context pool) blank shares of 1/8 and 1/32: the drop on, and off"""
    _run_all(out_json, [(n, True, True) for n in SPARSE] + [(n, False, False) for n in SPARSE], debug_build=False)


def _run_debug(out_json):
    """(child on the bounds-checking build with WP_ARENA_GUARD=1) every named case, and the sparse filler"""
    _run_all(out_json, [(n, True, None) for n in NAMED] + [(n, False, None) for n in SPARSE], debug_build=True)
    overflow_case()
    handle_reuse()


def _run_all(out_json, runs, debug_build):
    """the outcome of each run goes to out_json as it comes.  An error that is no failed comparison ends the run: nothing is
    started on the GPU behind it."""
    results = {}
    for name, dense, drop in runs:
        key, stop = "%s/%d" % (name, dense), False
        try:
            check_case(name, dense, drop, debug_build)
            results[key] = "ok"
        except AssertionError:
            results[key] = traceback.format_exc()[-2000:]
        except Exception:
            results[key] = traceback.format_exc()[-2000:]
            stop = True
        with open(out_json, "w") as f:
            json.dump(results, f)
        if stop:
            raise RuntimeError("stopped behind %s" % key)
    bad = {k: v for k, v in results.items() if v != "ok"}
    assert not bad, bad


def _child(tmp_path, func, env, n_runs):
    out = tmp_path / "results.json"
    r = R.run_in_child(tmp_path, "test_gpu_early_refine", func, (str(out),), env, timeout=900, check=False)
    results = {}
    if out.exists():
        with open(str(out)) as f:
            results = json.load(f)
    bad = {k: v for k, v in results.items() if v != "ok"}
    tail = "child ended with %d: %s %s" % (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    assert not bad and len(results) == n_runs and r.returncode == 0 and "CHILD_OK" in r.stdout, \
        "\n".join("%s: %s" % kv for kv in sorted(bad.items())[:4]) + tail


def test_blank_drop_on_and_off(tmp_path):
    """A blank share on each side of kBlankDropMinShare = 1/16, every handle with a symbol code of its own: with the drop
    the groups' first slots are slots of the shorter sorted array (round0_sorted = the kept suffixes)."""
    assert 1 / 32 < R.BLANK_DROP_MIN_SHARE < 1 / 8
    _child(tmp_path, "_run_blank_shares", {"WP_NO_CONTEXT_POOL": "1"}, 2 * len(SPARSE))


def test_early_refine_bounds_build(tmp_path):
    """The named cases, the overflow input and the handle-reuse sequence in the bounds-checking build with a guard zone
    behind every arena allocation: a non-zero site counter (kSiteCandRun, kSiteListSlot, kSiteRankStore, kSiteKeyStep ...)
    or a damaged zone makes the encode fail."""
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    _child(tmp_path, "_run_debug", {"WP_LIB": dbg, "WP_ARENA_GUARD": "1"}, len(NAMED) + len(SPARSE))


# ---- the list overflow ---------------------------------------------------------------------------------------------------

def _periodic(n_words):
    words = [b"ab" * 40, b"ab" * 33 + b"c", b"ba" * 25]
    rng = random.Random(77)
    text = b" ".join(rng.choice(words) for _ in range(n_words))
    vocab = ["[UNK]"] + ["ab" * k for k in (1, 2, 5, 9, 14, 20, 33, 40)] + ["##" + "ab" * k for k in (1, 3, 7, 12, 21)] + \
            ["ba" * k for k in (1, 4, 11, 25)] + ["##c", "##b", "##a", "a", "b"]
    return text, vocab


def overflow_case():
    """The overflow input of test_gpu_keys_only_sort.py, rebuilt: a periodic text whose every suffix shares its key with long
    tokens.  The needed list outgrows its first room while the passes run; the retry takes the early path again."""
    text, vocab = _periodic(70_000)
    gv = W.Vocab(vocab)
    ids = gv.encode(text)
    st, rs, sched = gv.stats(), gv.refine_stats(), gv.refine_sched()
    print({k: st[k] for k in ("n_total", "round0_candidates", "needed_after_round0", "list_retries")}, rs, sched, flush=True)
    assert st["round0_keys_only"] == 1 and st["list_retries"] == 1 and sched["early"] == 1, (st, sched)
    ref = _handle(vocab, W.WP_OPT_INDEXED_ROUND0)
    assert np.array_equal(ids, ref.encode(text)), "ids of the retried encode against the indexed handle"
    late = _handle(vocab, W.WP_OPT_LATE_REFINE)
    assert np.array_equal(ids, late.encode(text)) and late.stats()["list_retries"] == 1 and late.refine_stats() == rs
    assert np.array_equal(gv.encode(text), ids) and gv.stats()["list_retries"] == 0 and gv.refine_sched()["early"] == 1


def test_list_overflow_retries_on_the_early_path():
    overflow_case()


def test_list_of_2_22_entries_takes_the_partitioned_store():
    """The same periodic text with 90,000 words: more than 2^22 list entries, where the slot base is added in place
    (list_rank_base_kernel) and the ranks go through the partitioned store.  Ids against both other placements."""
    text, vocab = _periodic(90_000)
    gv = W.Vocab(vocab)
    ids = gv.encode(text)
    rs, sched = gv.refine_stats(), gv.refine_sched()
    print(rs, sched, flush=True)
    assert rs["n_entries"] >= 1 << 22 and sched["early"] == 1 and gv.stats()["round0_keys_only"] == 1, (rs, sched)
    late = _handle(vocab, W.WP_OPT_LATE_REFINE)
    assert np.array_equal(ids, late.encode(text)) and late.refine_stats() == rs and late.refine_sched()["early"] == 0
    assert np.array_equal(ids, _handle(vocab, W.WP_OPT_INDEXED_ROUND0).encode(text))


# ---- one handle, unlike texts ----------------------------------------------------------------------------------------------

def handle_reuse():
    """8 encodes through one handle: texts with needed groups and texts with none in turn, above and below RADIX_SMALL_N,
    one of them with more than 255 code points (32-bit symbols: round 0 keeps its index column, nothing runs early)"""
    c = K.build("L_three_large")
    vocab = vocab_of(c)
    fill = filler(True)
    texts = [embed(c), fill, c.text, fill[:70_000] + b" jk", embed(c, dense=False), c.text + b" " + K.WIDE_FILL.encode("utf-8"),
             K.between_text(c), filler(False)[1000:]]
    entries = [sum(f.k for f in c.families), 0, sum(f.k for f in c.families), 0, sum(f.k for f in c.families),
               sum(f.k for f in c.families), None, 0]
    early = [1, 1, 1, 1, 1, 0, 1, 1]
    ov, gv = O.Vocab(vocab), W.Vocab(vocab)
    for i, text in enumerate(texts):
        ids = gv.encode(text)
        st, rs, sched = gv.stats(), gv.refine_stats(), gv.refine_sched()
        print(i, len(text), st["round0_keys_only"], rs["n_entries"], sched, flush=True)
        assert np.array_equal(ids, ov.encode(text, threads=8)), (i, "ids")
        assert sched["early"] == early[i] == st["round0_keys_only"], (i, sched, st["round0_keys_only"])
        if entries[i] is not None:
            assert rs["n_entries"] == entries[i], (i, rs)
        else:
            assert rs["n_entries"] > 0, (i, rs)


def test_handle_reuse_with_and_without_needed_groups():
    handle_reuse()


# ---- byte offsets from the device entry point ---------------------------------------------------------------------------------

def test_byte_offsets_from_the_device_entry_point():
    """wp_linear_encode_offsets_device reads the same ranks: ids against the oracle, every span of a known id spells its
    token, and the spans equal those of the (key, index) sort"""
    import torch
    name = "L_three_large"
    text, vocab, exp = reference(name)
    t = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    gv = W.Vocab(vocab)
    ids, offs = gv.encode_tensor(t, offsets=True, unit="byte")
    assert gv.refine_sched()["early"] == 1 and gv.stats()["offsets_unit"] == W.WP_OFFSETS_BYTES
    ids, offs = ids.cpu().numpy(), offs.cpu().numpy().astype(np.int64).reshape(-1, 2)
    assert np.array_equal(ids, exp), "ids of the offsets call"
    unk = vocab.index("[UNK]")
    for k in range(len(ids)):
        if ids[k] != unk:
            tok = vocab[ids[k]]
            assert text[offs[k, 0]:offs[k, 1]].decode("utf-8") == (tok[2:] if tok.startswith("##") else tok), (k, tok, offs[k])
    iv = _handle(vocab, W.WP_OPT_INDEXED_ROUND0)
    ids_i, offs_i = iv.encode_tensor(t, offsets=True, unit="byte")
    assert np.array_equal(ids_i.cpu().numpy(), exp) and np.array_equal(offs_i.cpu().numpy().astype(np.int64).reshape(-1, 2), offs)
