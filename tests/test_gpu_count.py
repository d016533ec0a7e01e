"""GPU checks of the word counts (wp_count_words, wp_count_words_device) against tests/count_model.py, exactly: the bytes
of the pool, the offsets, the counts, the per-occurrence index and the statistics — at the tile edges of the word-start
pass, at the limits of the rules, through the collision rounds, at the sizes where the sorts change configuration, end to
end with the encoder, and across the states of a handle."""
import os
import random
import re
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

import count_model as CM
import wordpiece_amd as W
from wordpiece_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")
VOCAB = ["[UNK]", "a", "b", "##b", "中", "."]
T = 2048  # the tile of the word-start pass (count.h: kCountTile)
STAT_KEYS = ("n_words", "n_distinct", "n_long", "n_below_min", "n_text_bytes")


def test_geometry_matches_the_kernels():
    src = open(os.path.join(PKG, "csrc", "count.h")).read()
    common = open(os.path.join(PKG, "csrc", "common.h")).read()
    block = int(re.search(r"constexpr int kBlock = (\d+);", common).group(1))
    assert block * int(re.search(r"constexpr int kCountItems = (\d+);", src).group(1)) == T
    assert re.search(r"constexpr int kCountTile = kBlock \* kCountItems;", src)
    assert re.search(r"kSiteCount = 15,", common)
    radix = open(os.path.join(PKG, "csrc", "radix_sort.h")).read()
    assert re.search(r"constexpr size_t kRadixSmallN = size_t\(1\) << 21;", radix)


_handles = {}


def handle(flags=0):
    if flags not in _handles:
        _handles[flags] = W.Vocab(VOCAB, normalize=flags)
    return _handles[flags]


def check(text, where, flags=0, index=True, tensor=False, v=None, **kw):
    """one call against the model; -> (the model's table, the statistics of the call)"""
    import torch
    v = v or handle(flags)
    text = text if isinstance(text, (bytes, bytearray)) else text.encode("utf8")
    exp = CM.count_words(text, flags, **kw)
    if tensor:
        t = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda() if text else torch.zeros(0, dtype=torch.uint8, device="cuda")
        got = {k: x.cpu().numpy() for k, x in v.count_words_tensor(t, index=index, **kw).items()}
    else:
        got = v.count_words(text, raw=True, index=index, **kw)
    assert got["words"].tobytes() == exp["pool"], where
    assert got["word_off"].dtype == np.int64 and got["word_off"].tolist() == exp["word_off"], where
    assert got["counts"].dtype == np.int64 and got["counts"].tolist() == exp["counts"], where
    assert ("word_index" in got) == index, where
    if index:
        assert got["word_index"].dtype == np.int32 and got["word_index"].tolist() == exp["word_index"], where
    st = v.count_stats()
    assert {k: st[k] for k in STAT_KEYS} == exp["stats"], where
    listed = exp["stats"]["n_words"] - exp["stats"]["n_long"]
    assert (st["n_rounds"] >= 1) == (listed > 0) and 0 <= st["n_collided"] <= max(listed - 1, 0), where
    return exp, st


def placed(pos, piece, tail=b" ab a"):
    """a text in which `piece` starts at byte `pos`, behind filler words and one blank"""
    piece = piece if isinstance(piece, bytes) else piece.encode("utf8")
    return (b"ab a " * (pos // 5 + 1))[:pos - 1] + b" " + piece + tail


@pytest.mark.gpu
def test_words_at_the_tile_edges():
    n = 0
    # a word from the first byte of a tile to its last (long under every bound), short ones that start / end there
    for piece in (b"q" * T, b"qrs", b"q"):
        for tensor in (False, True):
            check(placed(T, piece), ("first byte", len(piece)), tensor=tensor, max_word_bytes=1024)
    check(placed(2 * T - 3, b"qrs") + b"x" * 5, "ends on the last byte", max_word_bytes=8)
    # a word over one tile boundary, one over two (long)
    check(placed(T - 5, b"abcdefghij"), "straddles one")
    check(placed(T - 50, b"z" * (T + 100)) + placed(7, b"z" * 9), "straddles two", max_word_bytes=1024)
    # 2-, 3- and 4-byte characters over a boundary at each split: inside a word, as a word (CJK), behind punctuation
    for ch in ("é", "か", "中", "\U0001F600", "\U00020000"):
        size = len(ch.encode("utf8"))
        for cut in range(1, size):
            for piece in ("xy" + ch + "zw", ch, "." + ch + ch + ".", ch + " q"):
                lead = len(piece.split(ch)[0].encode("utf8"))
                check(placed(T - cut - lead, piece), ("split", ch, cut, piece), tensor=(n % 2 == 1))
                n += 1
    # a space / punctuation / CJK character as the last code point in front of a tile
    for last in (" ", "\n", "▁", ".", "—", "中", "\U00020000", "b"):
        piece = last + "xyz q"
        check(placed(T - len(last.encode("utf8")), piece), ("last before", last))
        check(placed(2 * T - len(last.encode("utf8")), piece, tail=b""), ("last before, open end", last), tensor=True)
    # the end of the text: inside a word, on a space, without any word, one word; the end of the text on a tile boundary
    for text in (b"ab cd", b"ab cd ", b" \n\t ", b"\xff\xfe", b"abc", b"a", b".", placed(T - 3, b"abc", tail=b""),
                 placed(T - 3, b"ab ", tail=b""), placed(T - 2, b"abc", tail=b""), b"a" * T, b"a" * (T - 1), b"a " * T):
        for tensor in (False, True):
            check(text, ("end", text[-8:], len(text)), tensor=tensor, max_word_bytes=1024)


@pytest.mark.gpu
def test_long_words_at_the_bound():
    for m in (1, 256, 1024):
        words = [b"a" * k for k in (m - 1, m, m + 1) if k > 0]
        words += [b"b" * (m - 1) + "é".encode(), "é".encode() + b"b" * (m - 1)]            # m + 1 bytes: the last character crosses the bound
        if m >= 2:
            words += [b"b" * (m - 2) + "é".encode(), b"c" * (m - 2) + "中".encode()]        # m bytes / m + 1 bytes
        if m >= 3:
            words += [b"c" * (m - 3) + "中".encode(), b"d" * (m - 3) + "\U0001F600".encode()]  # m bytes / m + 1 bytes
        text = b" ".join(words + words[::-1] + words[:2]) + b" . " + b" ".join(words)
        for tensor in (False, True):
            exp, st = check(text, ("bound", m), tensor=tensor, max_word_bytes=m, terminator=10)
            assert st["n_long"] > 0 and max(len(w) for w in exp["words"]) == m
    exp, _ = check(b"a" * 256 + b" " + b"a" * 257, "the default bound", max_word_bytes=0)
    assert exp["words"] == [b"a" * 256]


@pytest.mark.gpu
def test_min_count_orders_terminators_and_want():
    rng = random.Random(5)
    words = ["w%d" % k for k in range(40)] + ["中", ".", "é", "か"]
    text = " ".join(rng.choice(words[:8]) if rng.random() < 0.5 else rng.choice(words) for _ in range(700))
    counts = Counter(CM.split(text))
    assert len(set(counts.values())) < len(counts) - 10  # many ties
    some = sorted(set(counts.values()))[2]
    for order in ("first", "count"):
        for min_count in (0, 1, some - 1, some, some + 1, 10 ** 6):
            exp, st = check(text, (order, min_count), order=order, min_count=min_count, tensor=(min_count % 2 == 0))
        assert exp["words"] == [] and st["n_below_min"] == len(counts)
        for terminator in (None, 0, 10, 255):
            for index in (False, True):
                check(text, (order, terminator, index), order=order, terminator=terminator, index=index, tensor=index)
    v = handle()
    assert v.count_words(text, order="count")["words"] == [w.decode("utf8") for w, _ in counts.most_common()]
    assert v.count_words(text, terminator="\n")["words"] == [w.decode("utf8") for w in counts]


@pytest.mark.gpu
def test_normalised_text_and_invalid_bytes():
    text = "Caf\u00e9 cafe CAFE  caf\u00e9s Ca\u200bf\u00e9 na\u00efve NA\u00cfVE \u4e2dA\u4e2da\u00a0\u01c4 \u01c6. \u0130".encode("utf8")
    for flags in range(8):
        for tensor in (False, True):
            exp, _ = check(text, ("flags", flags), flags=flags, tensor=tensor, order="count")
    exp, _ = check(text, "uncased", flags=W.WP_NORM_BERT_UNCASED)
    assert exp["words"][0] == b"cafe" and exp["counts"][0] == 4
    # invalid UTF-8 inside a word, at its ends, at a tile boundary: dropped, the word goes on
    bad = b"ab\xffcd ab\xc3cd \xe4\xb8ab cd\xf0\x9f\x98 abcd \x80 \xed\xa0\x80x"
    for tensor in (False, True):
        exp, _ = check(bad, "invalid", tensor=tensor)
        assert exp["words"][0] == b"abcd" and exp["counts"][0] == 3
        check(placed(T - 2, b"ab\xff\xfecd"), "invalid at a tile boundary", tensor=tensor)


@pytest.mark.gpu
def test_collision_rounds_never_change_a_result():
    rng = random.Random(6)
    words = ["%s%d" % (rng.choice(("k", "kk", "中", "é")), k) for k in range(600)]
    text = " ".join(rng.choice(words[:50]) if rng.random() < 0.4 else rng.choice(words) for _ in range(3000)) + " " + " ".join(words)
    v = handle()
    results = {}
    for bits in (8, 12, 64, 0):
        for order in ("first", "count"):
            exp, st = check(text, ("hash_bits", bits, order), order=order, hash_bits=bits, terminator=10)
            assert st["n_distinct"] == len(set(CM.split(text))) >= 600
            results[bits, order] = (v.count_words(text, raw=True, index=True, order=order, hash_bits=bits), st)
        if bits == 8:
            assert st["n_rounds"] > 1 and st["n_collided"] > 0
        if bits in (64, 0):
            assert st["n_rounds"] == 1 and st["n_collided"] == 0
    for order in ("first", "count"):
        for bits in (12, 64, 0):
            for key in ("words", "word_off", "counts", "word_index"):
                assert np.array_equal(results[bits, order][0][key], results[8, order][0][key]), (bits, order, key)


def _ascii_words(text):
    return re.findall(rb"[A-Za-z0-9]+|[^\sA-Za-z0-9]", text)


def _check_big(text, words, order):
    """a large ASCII text against Counter on the host, through the tensor form"""
    import torch
    cnt = Counter(words)
    pairs = cnt.most_common() if order == "count" else list(cnt.items())
    v = handle()
    got = v.count_words_tensor(torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda(), order=order, index=True, copy=False)
    lens = np.fromiter((len(w) for w, _ in pairs), dtype=np.int64, count=len(pairs))
    assert got["words"].cpu().numpy().tobytes() == b"".join(w for w, _ in pairs)
    assert np.array_equal(got["word_off"].cpu().numpy(), np.concatenate(([0], np.cumsum(lens))))
    assert np.array_equal(got["counts"].cpu().numpy(), np.fromiter((c for _, c in pairs), dtype=np.int64, count=len(pairs)))
    slot = {w: k for k, (w, _) in enumerate(pairs)}
    assert np.array_equal(got["word_index"].cpu().numpy(), np.fromiter((slot[w] for w in words), dtype=np.int32, count=len(words)))
    st = v.count_stats()
    assert (st["n_words"], st["n_distinct"], st["n_long"], st["n_text_bytes"]) == (len(words), len(pairs), 0, len(text))
    return st


@pytest.mark.gpu
def test_more_words_than_the_small_sort_takes():
    text, _ = synth.english_corpus(14_000_000, seed=3, vocab_size=200, lexicon_size=30000)
    assert max(text) < 128 and not re.search(rb"[\x00-\x08\x0e-\x1f\x7f]", text)
    words = _ascii_words(text)
    assert len(words) > 2 ** 21
    _check_big(text, words, "count")


@pytest.mark.gpu
def test_more_distinct_words_than_the_small_sort_takes():
    n = 2 ** 21 + 5000
    text = (" ".join(map(str, range(n))) + " " + " ".join(map(str, range(0, n, 997))) + " 5 5").encode()
    words = text.split()
    st = _check_big(text, words, "count")
    assert st["n_distinct"] == n > 2 ** 21
    _check_big(text, words, "first")


@pytest.mark.gpu
def test_pool_through_the_encoder_equals_the_encode():
    import torch
    text, vocab = synth.english_corpus(200_000, seed=1, vocab_size=3000)
    # no token that holds a spacing character beside others: the encoder's words are then the words of the table
    vocab = [t for t in vocab if len(t[2:] if t.startswith("##") else t) == 1 or not any(CM.spacing(ord(ch)) for ch in t.lstrip("#"))]
    v = W.Vocab(vocab)
    t = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    table = v.count_words_tensor(t, terminator="\n", index=True)
    ids, splits = v.encode_rows_tensor(table["words"], table["word_off"])
    ids, splits = ids.cpu().numpy(), splits.cpu().numpy()
    counts, index = table["counts"].cpu().numpy(), table["word_index"].cpu().numpy()
    assert len(splits) == len(counts) + 1 and index.min() >= 0
    per_word = np.diff(splits)
    want = v.encode_tensor(t).cpu().numpy()
    assert int((counts * per_word).sum()) == len(want)
    lens = per_word[index]
    starts = np.repeat(splits[:-1][index] - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()))
    assert np.array_equal(ids[starts], want)


@pytest.mark.gpu
def test_handle_state():
    import torch
    text = ("b a b . 中 ab a b " * 40).encode("utf8")
    v = W.Vocab(VOCAB)
    assert v.count_stats()["n_words"] == -1
    exp, _ = check(text, "first call", v=v)
    ids = v.encode(text)
    assert len(ids) == 9 * 40 and v.count_stats()["n_words"] == -1  # (an encode since: as every layer's statistics)
    check(text + b" q", "after an encode", v=v, tensor=True, order="count")
    assert v.encode(text).tolist() == ids.tolist()
    # another vocabulary, the same table
    other = W.Vocab(["x", "b a", "[MASK]", "##.", "中ab"])
    a, b = v.count_words(text, raw=True, index=True), other.count_words(text, raw=True, index=True)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # views live until the handle's next call, whatever other handles do
    t = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    views = v.count_words_tensor(t, index=True, copy=False, terminator=0)
    kept = {k: x.clone() for k, x in views.items()}
    other.count_words_tensor(t, order="count")
    other.encode(text)
    assert all(torch.equal(views[k], kept[k]) for k in views)
    copies = v.count_words_tensor(t, index=True, terminator=0)
    assert all(torch.equal(copies[k], kept[k]) for k in kept)
    # sizes up and down around trim
    for size, trim in ((3, False), (5000, False), (2, True), (900, False)):
        if trim:
            v.trim()
        check(b"ab " * size, ("sizes", size, trim), v=v, tensor=trim)


@pytest.mark.gpu
def test_bounds_checking_build(tmp_path):
    """(child on the bounds-checking build with WP_ARENA_GUARD=1; the host form, whose device half is the device form's) tile edges, long words, the collision rounds and both
    orders: no store or gather outside an array (kSiteCount, kSiteGroup), no guard zone of the call's arenas overwritten"""
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "count_dbg_run.py"
    script.write_text('''
import random, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import wordpiece_amd as W
from test_gpu_count import T, check, handle, placed
v = handle()
v.encode("ab a")
assert v.stats()["reserved0"] == 1, "not the bounds-checking build"
rng = random.Random(51)
words = ["k%%d" %% k for k in range(300)] + ["\\u4e2d", ".", "q" * 300]
text = " ".join(rng.choice(words) for _ in range(2500))
for bits in (8, 64):
    for order in ("first", "count"):
        exp, st = check(text, "debug", order=order, hash_bits=bits, terminator=10, min_count=2)
        assert st["n_long"] > 0 and (bits == 64 or st["n_rounds"] > 1)
check(placed(T - 1, "\\u4e2dxy"), "debug tile")
check(b"", "debug empty")
check(b"  ", "debug no word")
print("COUNT_DEBUG_OK")
''' % (os.path.dirname(PKG), HERE))
    env = dict(os.environ, WP_LIB=dbg, WP_ARENA_GUARD="1")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "COUNT_DEBUG_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
