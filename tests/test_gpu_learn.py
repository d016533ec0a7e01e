"""The vocabulary learner on the device (wp_learn_vocab, wp_learn_vocab_device) against its model (learn_model.py):
every call is compared exactly — the tokens in order, their scores, the threshold, the steps of the search and the
statistics.  Tables stay small: the model is plain Python."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import count_model as CM
import learn_model as M
import wordpiece_amd as W

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(os.path.abspath(W.__file__))
RES = ("[PAD]", "[UNK]")
MODEL_STATS = ("n_words", "n_reserved", "n_long", "n_char_dropped", "n_chars", "n_occurrences", "n_tokens", "n_steps", "thresh")
_handle = []


def handle():
    if not _handle:
        _handle.append(W.Vocab(["[UNK]", "a", "##b", "ab", "c"], device=0))
    return _handle[0]


def pooled(words, terminator=None):
    term = b"" if terminator is None else terminator.encode()
    off = np.zeros(len(words) + 1, dtype=np.int64)
    if words:
        off[1:] = np.cumsum([len(w) + len(term) for w in words])
    return np.frombuffer(b"".join(w + term for w in words), dtype=np.uint8), off


def run(words, counts, tag, vocab_size, v=None, tensor=False, terminator=None, reserved=RES, **kw):
    """words: bytes each.  -> (the model's result, the statistics of the device call)"""
    v = v or handle()
    kw.setdefault("lower_thresh", 1)
    kw.setdefault("upper_thresh", 64)
    kw.setdefault("max_token_chars", 8)
    kw.setdefault("slack", 2)
    hash_bits = kw.pop("hash_bits", 0)
    exp = M.learn(words, counts, vocab_size, reserved=[r.encode() for r in reserved], **kw)
    size = len(exp["tokens"])
    pool, off = pooled(words, terminator)
    args = dict(kw, reserved=reserved, hash_bits=hash_bits)
    if tensor:
        dev = torch.device("cuda", 0)
        r = v.learn_vocab_tensor(torch.from_numpy(pool.copy()).to(dev), torch.from_numpy(off).to(dev),
                                 torch.tensor(counts, dtype=torch.int64, device=dev), vocab_size, terminator=terminator, **args)
        data = bytes(r["tokens"].cpu().numpy())
        toff = r["token_off"].tolist()
        assert toff[0] == 0 and toff[-1] == len(data), tag
        got = dict(tokens=[data[a:b - 1].decode("utf8") for a, b in zip(toff, toff[1:])], scores=r["scores"].tolist(), thresh=r["thresh"])
        assert all(data[b - 1] == 10 for b in toff[1:]), tag
    else:
        r = v.learn_vocab({"words": pool, "word_off": off, "counts": counts, "terminator": terminator}, vocab_size, **args)
        got = dict(tokens=r["tokens"], scores=r["scores"].tolist(), thresh=r["thresh"])
    st = v.learn_stats()
    assert got["tokens"] == exp["tokens"], (tag, got["tokens"][:40], exp["tokens"][:40])
    assert got["scores"] == exp["scores"], (tag, got["scores"][:40], exp["scores"][:40])
    assert got["thresh"] == exp["thresh"] and len(got["tokens"]) == size, tag
    assert {k: st[k] for k in MODEL_STATS} == {k: exp["stats"][k] for k in MODEL_STATS}, (tag, st, exp["stats"])
    return exp, st


def enc(words):
    return [w.encode("utf8") if isinstance(w, str) else w for w in words]


def random_table(seed, n_words, alphabet="abcdefgh", max_len=8, max_count=40):
    rng = random.Random(seed)
    words = set()
    while len(words) < n_words:
        words.add("".join(rng.choice(alphabet) for _ in range(rng.randint(1, max_len))))
    words = sorted(words)
    rng.shuffle(words)
    return enc(words), [rng.randint(1, max_count) for _ in words]


@pytest.mark.gpu
def test_worked_example():
    words, counts = enc(["the", "then", "hen", "cat", "cats", "a", "at"]), [10, 4, 3, 5, 2, 7, 3]
    for size, thresh, n in ((20, 4, 19), (30, 1, 22)):
        for tensor in (False, True):
            exp, st = run(words, counts, ("example", size), size, upper_thresh=10, slack=1, tensor=tensor)
            assert (exp["thresh"], len(exp["tokens"])) == (thresh, n) and st["n_rounds"] == 1 and st["n_collided"] == 0
    assert exp["tokens"][-6:] == ["the", "cat", "then", "hen", "at", "cats"]


@pytest.mark.gpu
def test_character_cases():
    # words of max_token_chars and one more; the longer one is dropped and its characters with it
    exp, st = run(enc(["abcde", "abcdef", "xyzuvw", "ab"]), [5, 9, 9, 2], "max chars", 30, max_token_chars=5)
    assert st["n_long"] == 2 and "x" not in exp["tokens"] and "abcde" in exp["tokens"]
    # characters of 2, 3 and 4 bytes: lengths are code points, the list is in code point order
    words = enc(["é日😀", "日é", "😀😀é", "aé日", "日日日日"])
    exp, st = run(words, [7, 3, 4, 2, 6], "wide characters", 40, max_token_chars=4)
    assert st["n_chars"] == 4 and exp["tokens"][2:10] == ["a", "##a", "é", "##é", "日", "##日", "😀", "##😀"] and "日日日日" in exp["tokens"]
    # 64 characters of 4 bytes: the longest word there can be
    run(enc(["😀" * 64, "😀" * 3]), [2, 5], "longest word", 20, max_token_chars=64, upper_thresh=8)
    # one-character words only, and a single word
    exp, st = run(enc(list("abcab")), [1, 2, 3, 4, 5], "single characters", 20)
    assert st["n_occurrences"] == 5 and st["n_tokens"] == 3 and exp["scores"][2:8] == [5, 1, 7, 1, 3, 1]
    run(enc(["word"]), [3], "a single word", 12, upper_thresh=4)
    run(enc(["w"]), [1], "a single character", 12, upper_thresh=1)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_item_counts_at_the_wave_and_tile_edges(n):
    # n one-character words are n items: either side of the wave of the segmented sum and of the tile of the enumeration
    words, counts = enc(["abcde"[k % 5] for k in range(n)]), [1 + k % 7 for k in range(n)]
    exp, st = run(words, counts, ("items", n), 20)
    assert st["n_occurrences"] == n and st["n_tokens"] == 5
    # ... and the same number of items from words of two characters (3 items each) and single characters behind them
    k, rest = divmod(n, 3)
    words = enc([("ab", "bc", "ca", "ba")[j % 4] for j in range(k)] + ["c"] * rest)
    exp, st = run(words, [1 + j % 5 for j in range(k + rest)], ("items in words", n), 30, upper_thresh=256)
    assert st["n_occurrences"] == n


@pytest.mark.gpu
def test_group_larger_than_a_tile():
    # one letter in 5,000 words: its group has more members than a workgroup's tile, and its sum crosses many waves
    abc = "abcdefghijklmnopqrst"
    words = enc(["e" + abc[k % 20] + abc[k // 20 % 20] + abc[k // 400] for k in range(5000)])
    counts = [1 + k % 3 for k in range(5000)]
    exp, st = run(words, counts, "hot group", 200, upper_thresh=4096, slack=40, num_iterations=2)
    assert st["n_occurrences"] == 50000 and exp["scores"][exp["tokens"].index("e")] >= 1


@pytest.mark.gpu
def test_counts_beyond_32_bits():
    words, counts = random_table(7, 40, alphabet="abcd", max_len=5)
    counts = [c << 40 for c in counts]
    exp, st = run(words, counts, "wide counts", 40, lower_thresh=1 << 40, upper_thresh=1 << 50, slack=3)
    assert exp["thresh"] >= 1 << 40 and max(exp["scores"]) >= 1 << 41


@pytest.mark.gpu
def test_collision_rounds_change_nothing():
    words, counts = random_table(11, 300, max_len=6)
    exp, st = run(words, counts, "64 bits", 150, slack=8)
    assert st["n_rounds"] == 1 and st["n_collided"] == 0
    exp8, st8 = run(words, counts, "8 bits", 150, slack=8, hash_bits=8)
    assert st8["n_rounds"] > 1 and st8["n_collided"] > 0 and exp8["tokens"] == exp["tokens"]


@pytest.mark.gpu
def test_search_cases():
    words, counts = random_table(13, 80, max_len=6)
    run(words, counts, "lower == upper", 60, lower_thresh=7, upper_thresh=7)
    exp, st = run(words, counts, "below the characters", 3)  # the search runs to its end; the characters stay
    assert len(exp["tokens"]) >= 2 + 16 and st["n_steps"] > 1
    run(words, counts, "slack 0", 70, slack=0)
    for it in (1, 4):
        run(words, counts, ("iterations", it), 60, num_iterations=it, slack=0)
    run(words, counts, "defaults of the search", 60, lower_thresh=10, upper_thresh=10_000_000, slack=3, max_token_chars=50)


@pytest.mark.gpu
def test_max_unique_chars_with_ties():
    words = enc(["ab", "ba", "zb", "#a", "cab", "q"])
    for k in (1, 2, 3, 4, 5, 6, 7):
        exp, st = run(words, [1, 1, 1, 1, 2, 1], ("unique chars", k), 30, max_unique_chars=k)
    exp, st = run(words, [1] * 6, "ties", 30, max_unique_chars=3)  # a, b, then '#' before c, q and z on the tie
    assert st["n_char_dropped"] == 3 and st["n_chars"] == 3
    exp, st = run(enc(["ab", "ba"]), [1, 1], "every word dropped", 30, max_unique_chars=1)
    assert exp["tokens"] == list(RES) and st["n_char_dropped"] == 2 and st["n_steps"] == 0


@pytest.mark.gpu
def test_any_table_is_taken():
    # duplicates add up, empty words are skipped, reserved tokens and joiners are dropped; with and without a terminator
    words = enc(["ab", "", "abc", "[UNK]", "ab", "##ab", "#", "abc", ""])
    counts = [3, 9, 2, 50, 4, 60, 1, 0, 5]
    for term in (None, "\n"):
        for tensor in (False, True):
            exp, st = run(words, counts, ("any table", term, tensor), 20, terminator=term, tensor=tensor)
            assert st["n_reserved"] == 2 and exp["scores"][exp["tokens"].index("ab")] == 7
    merged, _ = run(enc(["ab", "abc", "#"]), [7, 2, 1], "merged", 20)
    assert merged["tokens"] == exp["tokens"] and merged["scores"] == exp["scores"]


@pytest.mark.gpu
def test_table_check_names_what_it_found():
    v = handle()
    good = {"words": np.frombuffer(b"abcd", dtype=np.uint8), "word_off": [0, 2, 4], "counts": [1, 1]}
    for change, msg in ((dict(word_off=[2, 1, 4]), "word_off descends or leaves the pool at word 0"),
                        (dict(word_off=[0, 0, 4], terminator="\n"), "word_off descends or leaves the pool at word 0"),
                        (dict(counts=[1, -1]), "count of word 1 is negative"),
                        (dict(words=np.frombuffer(b"ab\xc3d", dtype=np.uint8)), "word 1 is not valid UTF-8"),
                        (dict(words=np.frombuffer(b"\xed\xa0\x80d", dtype=np.uint8), word_off=[0, 3, 4]), "word 0 is not valid UTF-8")):
        with pytest.raises(W.WordPieceError, match=msg):
            v.learn_vocab(dict(good, **change), 10)
    with pytest.raises(W.WordPieceError, match="word_off ends behind the pool"):
        v.learn_vocab(dict(good, word_off=[0, 2, 9]), 10)
    dev = torch.device("cuda", 0)
    with pytest.raises(W.WordPieceError, match="word_off descends or leaves the pool at word 1"):  # (the device form is told the pool's size)
        v.learn_vocab_tensor(torch.from_numpy(good["words"].copy()).to(dev), torch.tensor([0, 2, 9], device=dev), torch.tensor([1, 1], device=dev), 10)
    assert v.learn_vocab(good, 10, lower_thresh=1, upper_thresh=1)["tokens"][-2:] == ["ab", "cd"]


TEXT = "The cat, the cats and the hen: 中文 then 中 at the café — hen, cat! " * 3 + "naïve cafés that the hen then ate."


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["first", "count"])
def test_table_straight_from_the_count_call(order):
    v = handle()
    data = TEXT.encode("utf8")
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    for term in (None, "\n"):
        table = v.count_words_tensor(t, order=order, terminator=term, copy=False)
        r = v.learn_vocab_tensor(table["words"], table["word_off"], table["counts"], 60, reserved=RES, lower_thresh=1, upper_thresh=32,
                                 slack=3, terminator=term)
        cm = CM.count_words(data, order=order)
        exp = M.learn(cm["words"], cm["counts"], 60, reserved=[x.encode() for x in RES], lower_thresh=1, upper_thresh=32, slack=3)
        assert bytes(r["tokens"].cpu().numpy()).decode("utf8").split("\n")[:-1] == exp["tokens"]
        assert r["scores"].tolist() == exp["scores"] and r["thresh"] == exp["thresh"]
        assert "中" in exp["tokens"] and "," in exp["tokens"] and "the" in exp["tokens"]


@pytest.mark.gpu
def test_calls_leave_each_other_alone():
    v = W.Vocab(["[UNK]", "a", "##b", "ab", "c"], device=0)
    words, counts = random_table(17, 120, max_len=6)
    ids = v.encode("ab c abb").tolist()
    a, _ = run(words, counts, "first call", 90, v=v, slack=5)
    assert v.encode("ab c abb").tolist() == ids
    run(enc(["xy"]), [1], "a small call between", 10, v=v)
    b, _ = run(words, counts, "second call", 90, v=v, slack=5, tensor=True)
    assert a["tokens"] == b["tokens"] and v.encode("ab c abb").tolist() == ids
    assert v.learn_stats()["n_words"] == -1  # an encode since


@pytest.mark.gpu
def test_bounds_checking_build(tmp_path):
    """(child on the bounds-checking build with WP_ARENA_GUARD=1) the collision rounds, the character filter, wide
    characters, both forms and the empty results: no store or gather outside an array (kSiteLearn), no guard zone of the
    call's arenas overwritten"""
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "learn_dbg_run.py"
    script.write_text('''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import wordpiece_amd as W
from test_gpu_learn import enc, handle, random_table, run
v = handle()
v.encode("ab a")
assert v.stats()["reserved0"] == 1, "not the bounds-checking build"
words, counts = random_table(19, 400, alphabet="abcdef\\u00e9\\u65e5", max_len=7)
for bits in (8, 64):
    for tensor in (False, True):
        exp, st = run(words, counts, "debug", 200, slack=10, hash_bits=bits, max_unique_chars=6, tensor=tensor, terminator="\\n")
        assert st["n_char_dropped"] > 0 and (bits == 64 or st["n_rounds"] > 1)
run(enc(["\\U0001f600" * 64]), [2], "debug longest", 20, max_token_chars=64, upper_thresh=2)
run([], [], "debug empty", 10, tensor=True)
run(enc(["[PAD]", "##a"]), [1, 1], "debug all dropped", 10)
print("LEARN_DEBUG_OK")
''' % (os.path.dirname(PKG), HERE))
    env = dict(os.environ, WP_LIB=dbg, WP_ARENA_GUARD="1")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "LEARN_DEBUG_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_round_trip():
    """the learned vocabulary loads into the encoder: the text it came from encodes without [UNK] outside the words the
    filters dropped, and every word of the table encodes into the pieces of the model's greedy split"""
    text = TEXT + " " + "x" * 12 + " ##odd"
    kw = dict(lower_thresh=1, upper_thresh=32, slack=3, max_token_chars=10)
    v = W.learn_vocab(text, 70, **kw)
    boot = W.Vocab(["[UNK]"], device=0)
    table = boot.count_words(text, order="count")
    exp = M.learn(enc(table["words"]), table["counts"].tolist(), 70, **kw)
    assert len(v) == len(exp["tokens"]) and v.unk_id == exp["tokens"].index("[UNK]")
    vocab = set((t.startswith("##"), t[2:] if t.startswith("##") else t) for t in exp["tokens"][5:])
    index = {t: i for i, t in enumerate(exp["tokens"])}
    kept, _ = M.filter_words(enc(table["words"]), table["counts"].tolist(), [r.encode() for r in W.DEFAULT_RESERVED], 10, 1000)
    kept = [w for w, _ in kept]
    dropped = [w for w in table["words"] if w not in kept]
    assert "x" * 12 in dropped and len(dropped) <= 4
    # the table as one document per word, on the device
    t = torch.frombuffer(bytearray(text.encode("utf8")), dtype=torch.uint8).to("cuda:0")
    tt = boot.count_words_tensor(t, order="count", terminator="\n")
    ids, splits = v.encode_rows_tensor(tt["words"], tt["word_off"])
    ids, splits = ids.tolist(), splits.tolist()
    assert len(splits) == len(table["words"]) + 1
    for k, w in enumerate(table["words"]):
        row = ids[splits[k]:splits[k + 1]]
        if w in kept:
            starts = M.greedy_split(w, vocab) + [len(w)]
            assert row == [index[("##" if a else "") + w[a:b]] for a, b in zip(starts, starts[1:])], (w, row)
    # the text itself: [UNK] only where a dropped word stands
    n_unk = v.encode(text).tolist().count(v.unk_id)
    assert n_unk <= sum(int(c) for w, c in zip(table["words"], table["counts"]) if w in dropped)
