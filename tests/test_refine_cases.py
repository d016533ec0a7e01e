"""CPU checks of refine_cases.py: every case builds; its expected list (groups, entries, large groups) follows from a direct
count over the text; the oracle's ids equal the pure-Python models'; the oracle's per-slot best arrays, taken through its own
rank, equal refine_cases.longest_matches at every text position; the oracle's fast path equals its Linear path.

Wall time (measured on the build container): 110 s for the 202 cases, the three 4095- to 4097-group cases 7 s each."""
import numpy as np
import pytest

import bruteforce as BF
import offsets_model as OM
import oracle_lib as O
import refine_cases as K
import round0_cases as R
from test_gpu_parity import _combine

SMALL = 6000   # bytes of text up to which the quadratic brute-force model runs as well


def test_constants_and_table():
    """the constants come from the headers, and every named case stands in the table of the module's docstring"""
    assert K.LS_BITS == 10 and K.LS_GROUP_BITS == 12 and K.BLOCK == 256 and K.STEP_MAX_LEN == 2048 and K.BASE == K.KEY_BITS + 1
    assert len(K.names("F")) == K.F_SEEDS == 100
    doc = K.__doc__
    for name in K.names():
        group, rest = name.split("_", 1)
        stem = rest.rstrip("0123456789+-")
        assert name in doc or (stem and ("%s_%s" % (group, stem)) in doc) or ("_" + rest.split("_")[-1]) in doc, name
    for g in "GLTDRPNY":
        assert K.names(g), g
    assert all(n in K.names() for n in K.EMBEDDED)


def test_node_counts_of_the_pass_counts():
    """group N puts bit_length(trie_nodes + 1) on both sides of the sizes at which the window sort gains an LSD pass"""
    passes = lambda nodes: -(-(K.bit_length(nodes + 1) + K.LS_GROUP_BITS) // K.LS_BITS)
    got = [passes(K.expected_stats(K.build(n))[0]["trie_nodes"]) for n in K.names("N")]
    assert got == [2, 3, 3, 3, 4, 4], got


def check_case(name):
    c = K.build(name)
    refine, stats = K.expected_stats(c)
    text = c.text.decode("utf-8")
    # the expected list from a direct count: positions that share BASE symbols with a token of at least BASE symbols
    pops = {k: v for k, v in K.group_populations(c.text, c.vocab).items() if len(v) >= 2}
    sizes = sorted(len(v) for v in pops.values())
    assert len(sizes) == refine["n_groups"] and sum(sizes) == refine["n_entries"], (name, len(sizes), sum(sizes), refine)
    assert sorted(f.k for f in c.families if f.listed) == sizes, name
    assert sum(s > K.LS_MAXGROUP for s in sizes) == refine["n_large_groups"], name
    assert sum(s for s in sizes if s > K.LS_MAXGROUP) == refine["n_large_entries"], name
    assert (refine["symbol_bytes"] == 4) == (len(set(text) | set("".join(c.vocab))) > 255), name
    # a family's first symbol stands at its members' starts only (wide cases: the filler word holds every head once, with
    # another second symbol — two symbols of a wide code take at most 2 x 14 of the key's bits)
    for f in c.families:
        n_heads = text.count(f.head) - (K.WIDE_FILL.count(f.head) if refine["symbol_bytes"] == 4 else 0)
        assert n_heads == f.k, (name, f.head)
        if len(f.head) > 1 and refine["symbol_bytes"] == 1:
            assert text.count(f.head[0]) == sum(g.k for g in c.families if g.head[0] == f.head[0]), (name, f.head)
    if refine["symbol_bytes"] == 1 and any(len(f.head) > 1 for f in c.families):
        lens = R.code_lengths(c.text, c.vocab)
        worst = max(sum(lens[ord(ch)] for ch in f.head) for f in c.families) if lens else 2 * 8
        assert worst <= K.KEY_BITS, (name, worst)
    # ids: oracle == models
    ov = O.Vocab(c.vocab)
    exp = ov.encode(c.text)
    ids_m, spans, _, _ = OM.encode_spans(c.text, c.vocab)
    assert ids_m == exp.tolist(), name
    if len(c.text) <= SMALL and len(c.vocab) <= 200:
        assert BF.encode(c.text, c.vocab) == exp.tolist(), name
    # (no spacing char lies inside a token)
    assert np.array_equal(ov.fast_encode(c.text), exp), name
    # the oracle's best arrays through its own rank against the dict trie
    d = ov.encode_debug(c.text)
    lens = [O.lib().wpo_vocab_token_len(ov._h, i) for i in range(ov.size)]
    rank = d["rank"][:d["n_text"]]
    want_p, want_s = K.longest_matches(c.text, c.vocab)
    assert np.array_equal(_combine(d, lens, "prefix")[rank], np.array(want_p, dtype=np.int32)), name
    assert np.array_equal(_combine(d, lens, "suffix")[rank], np.array(want_s, dtype=np.int32)), name
    return c, exp


@pytest.mark.parametrize("name", K.names())
def test_refine_case(name):
    check_case(name)


@pytest.mark.parametrize("name", K.names("F"))
def test_refine_composed(name):
    check_case(name)


def test_between_text_is_another_population():
    for name in ("G_group_64", "L_three_large", "T_chain_8"):
        c = K.build(name)
        pops = [len(v) for v in K.group_populations(K.between_text(c), c.vocab).values()]
        assert (max(pops) > K.LS_MAXGROUP) == (name[0] == "G"), (name, pops)
