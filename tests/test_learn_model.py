"""The vocabulary learner's model (learn_model.py) against the worked example of the contract and against the properties
the contract implies, on seeded random tables.  No device."""
import math
import random

import pytest

import learn_model as M

EXAMPLE = ([b"the", b"then", b"hen", b"cat", b"cats", b"a", b"at"], [10, 4, 3, 5, 2, 7, 3])
EXAMPLE_KW = dict(reserved=(b"[PAD]", b"[UNK]"), max_token_chars=8, num_iterations=4, lower_thresh=1, upper_thresh=10, slack=1)
RESERVED = (b"[PAD]", b"[UNK]", b"[CLS]", b"[SEP]", b"[MASK]")
CHARS = "a ##a c ##c e ##e h ##h n ##n s ##s t ##t".split()


def random_table(seed, n_words=60, alphabet="abcdeé日", max_len=7, max_count=50, distinct_counts=False):
    rng = random.Random(seed)
    words = []
    while len(words) < n_words:
        w = "".join(rng.choice(alphabet) for _ in range(rng.randint(1, max_len)))
        if w not in words:
            words.append(w)
    counts = rng.sample(range(1, 10 * n_words), n_words) if distinct_counts else [rng.randint(1, max_count) for _ in words]
    return [w.encode("utf8") for w in words], counts


def test_worked_example():
    r = M.learn(*EXAMPLE, 20, **EXAMPLE_KW)
    assert (r["thresh"], r["stats"]["n_steps"], len(r["tokens"])) == (4, 4, 19)
    assert r["tokens"] == ["[PAD]", "[UNK]"] + CHARS + ["the", "cat", "then"]
    r = M.learn(*EXAMPLE, 30, **EXAMPLE_KW)
    assert (r["thresh"], len(r["tokens"])) == (1, 22)
    assert r["tokens"] == ["[PAD]", "[UNK]"] + CHARS + ["the", "cat", "then", "hen", "at", "cats"]
    assert r["scores"][:2] == [0, 0] and r["scores"][-6:] == [10, 5, 4, 3, 3, 2]


def test_filters_in_order_and_their_counters():
    words = [b"[UNK]", b"##ab", b"", b"abcdefghi", b"ab", b"ba", b"zb", b"#a"]
    kept, st = M.filter_words(words, [1] * 8, [b"[UNK]"], 8, 0)
    assert [w for w, _ in kept] == ["ab", "ba", "zb", "#a"] and (st["n_words"], st["n_reserved"], st["n_long"]) == (8, 2, 1)
    # a and b occur 3 times each, '#' and z once: the tie goes to the lower code point, so K = 3 drops the word with z alone
    kept, st = M.filter_words(words, [1] * 8, [b"[UNK]"], 8, 3)
    assert [w for w, _ in kept] == ["ab", "ba", "#a"] and st["n_char_dropped"] == 1
    for bad, msg in (([b"a", b"\xff"], "word 1 is not valid UTF-8"),):
        with pytest.raises(M.TableError, match=msg):
            M.filter_words(bad, [1, 1], [], 8, 0)
    with pytest.raises(M.TableError, match="count of word 0 is negative"):
        M.filter_words([b"a"], [-1], [], 8, 0)


@pytest.mark.parametrize("seed", range(4))
def test_every_word_splits_over_the_result(seed):
    words, counts = random_table(seed)
    r = M.learn(words, counts, 40, lower_thresh=1, upper_thresh=200, max_token_chars=6, max_unique_chars=5)
    vocab = set(r["tokens"])
    kept, _ = M.filter_words(words, counts, RESERVED, 6, 5)
    assert 0 < len(kept) < len(words)
    tokens = set((t.startswith("##"), t[2:] if t.startswith("##") else t) for t in vocab if not t.startswith("["))
    for w, _ in kept:
        starts = M.greedy_split(w, tokens) + [len(w)]
        for a, b in zip(starts, starts[1:]):
            assert ("##" if a else "") + w[a:b] in vocab


@pytest.mark.parametrize("seed", range(3))
def test_duplicated_words_equal_the_merged_table(seed):
    words, counts = random_table(seed, n_words=30)
    rng = random.Random(100 + seed)
    dup_w, dup_c = list(words), list(counts)
    for k in rng.sample(range(30), 10):  # a second entry of the word behind its first: the merged table keeps the first place
        dup_w.append(words[k])
        dup_c.append(rng.randint(1, 20))
        counts[k] += dup_c[-1]
    kw = dict(lower_thresh=1, upper_thresh=100, max_token_chars=7)
    a, b = M.learn(dup_w, dup_c, 50, **kw), M.learn(words, counts, 50, **kw)
    assert (a["tokens"], a["scores"], a["thresh"]) == (b["tokens"], b["scores"], b["thresh"])


@pytest.mark.parametrize("seed", range(3))
def test_word_order_matters_only_through_the_tie_rule(seed):
    words, counts = random_table(seed, n_words=40, distinct_counts=True)
    order = list(range(40))
    random.Random(200 + seed).shuffle(order)
    kw = dict(lower_thresh=1, upper_thresh=400, max_token_chars=7)
    a = M.learn(words, counts, 60, **kw)
    b = M.learn([words[k] for k in order], [counts[k] for k in order], 60, **kw)
    assert a["thresh"] == b["thresh"] and sorted(zip(a["tokens"], a["scores"])) == sorted(zip(b["tokens"], b["scores"]))
    assert a["scores"] == b["scores"]  # the order by score is the same; only equal scores may trade places


@pytest.mark.parametrize("upper", [1, 7, 64, 10_000_000])
def test_search_ends_in_log_steps(upper):
    words, counts = random_table(5, n_words=20)
    for size in (1, 25, 40, 10_000):
        r = M.learn(words, counts, size, lower_thresh=1, upper_thresh=upper, slack=0, max_token_chars=7)
        assert 1 <= r["stats"]["n_steps"] <= math.log2(upper) + 2
        assert 1 <= r["thresh"] <= upper


def test_empty_and_all_dropped_tables_give_the_reserved_tokens():
    for words, counts in (([], []), ([b"[PAD]", b"##x", b""], [3, 2, 1])):
        r = M.learn(words, counts, 10, reserved=(b"[PAD]", b"[UNK]"))
        assert (r["tokens"], r["scores"], r["thresh"], r["stats"]["n_steps"]) == (["[PAD]", "[UNK]"], [0, 0], 0, 0)
