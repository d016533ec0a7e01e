"""GPU tests (-m gpu) of what a handle's context carries from one encode to the next (csrc/linear_path.h,
symbols_and_keys: the symbol code cached for kCodeReuse = 64 encodes and reused whenever alphabet size and bit width
match, the blanks' share that is refreshed only with the code; csrc/context.h, park_context: a parked context keeps
both): more than 70 encodes of different texts through one handle — encode, encode_with_offsets, encode_batch and
encode_stream mixed — each compared with the oracle and with a fresh handle; the two orders in which a stale share can
meet a text (drop on with nothing to drop, drop off on a blank-heavy text); the cached code on a text whose dominant
symbol had frequency zero when it was built; 32-bit symbols in between; a handle of another vocabulary that inherits
the cache from the pool, against WP_NO_CONTEXT_POOL=1.  Any order-preserving code is correct for any text and the blank
table is made from the current alphabet, so none of this may change an id; round0_sorted is the kept count or n_total,
nothing else.  The sequence runs once more in the bounds-checking build (kSiteSortOrder among its counters)."""
import functools
import os

import numpy as np
import pytest

import oracle_lib as O
import round0_cases as R
import wordpiece_amd as W
from round0_cases import RADIX_SMALL_N, TILE

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(os.path.abspath(W.__file__))

CYRILLIC = str.maketrans("etaon", "етаон")  # (Cyrillic letters: other code points, the same number of them)
N_BIG = RADIX_SMALL_N + 7 * TILE + 77       # above kRadixSmallN: the builder's histogram and the drop are possible


@functools.lru_cache(maxsize=None)
def _vocab():
    """Every character of every text below (except the wide one's) occurs in the vocabulary, so the alphabet of an encode
    — text plus vocabulary plus separator — has one size whatever the text: the cached code is reused every time."""
    vocab, words = R.edge_vocab(7)
    cyr = [w.translate(CYRILLIC) for w in words[:400]]
    vocab = sorted(set(vocab + cyr + ["##" + w for w in cyr[:50]] + list("етаоня") + ["я" * k for k in (2, 3, 7, 40)] +
                       [b + words[k] for k, b in enumerate(R.BLANKS)]))
    return vocab, words


@functools.lru_cache(maxsize=None)
def _texts():
    vocab, words = _vocab()
    dotted = [w + "." for w in words]
    blank = R.sized_text(90, words, N_BIG - 1, (N_BIG - 1) // 4)
    wide = "".join(chr(c) for c in range(0x100, 0x100 + 300) if chr(c).isalpha())
    rng = np.random.default_rng(91)
    dom = rng.choice(np.array([ord(c) for c in "я " + R.LETTERS], dtype=np.uint32), size=N_BIG - 1,
                     p=np.array([55, 20] + [25 / 26] * 26) / 100.0).astype("<u4").tobytes().decode("utf-32-le")
    return {
        "blank": blank,                                                # blank-heavy, above kRadixSmallN
        "noblank": R.sized_text(92, dotted, N_BIG - 1, 0),             # not one blank, the same size of alphabet
        "cyrillic": blank.decode().translate(CYRILLIC).encode(),       # the same words, five letters other code points
        "dominant": dom.encode(),                                      # a symbol no earlier text holds, above half of this one
        "small": R.sized_text(93, words, 300_000, 50_000),             # below kRadixSmallN
        "tile": R.sized_text(94, words, TILE - 100, TILE // 5),        # below one tile
        "empty": b"",
        "blanks": b" \t\n \r\v\f  ",
        "wide": (blank[:200_000].decode() + wide + blank[200_000:N_BIG // 2].decode()).encode(),  # 256+ code points: 32-bit symbols
    }


@functools.lru_cache(maxsize=None)
def _expected(key):
    return O.Vocab(_vocab()[0]).encode(_texts()[key], threads=8)


ORDER = ("blank", "noblank", "cyrillic", "small", "dominant", "tile", "empty", "wide", "blanks")
ROUNDS = 8  # 72 encodes: past kCodeReuse, so the code is rebuilt in the middle of the sequence, on whichever text is next


def run_sequence(expected, order=ORDER, rounds=ROUNDS, debug_build=False):
    """`rounds` times the texts of `order` through one handle, the entry point changing with every call; every result
    against expected(key) and a fresh handle's; returns the statistics of the single-text calls as (key, stats)"""
    vocab, _ = _vocab()
    texts = _texts()
    gv = W.Vocab(vocab)
    seen, fresh, count = [], {}, 0
    seq = [k for _ in range(rounds) for k in order]
    i = 0
    while i < len(seq):
        api = (i // 2) % 4
        keys = seq[i:i + 2] if api >= 2 else seq[i:i + 1]
        if api == 0:
            got = [gv.encode(texts[keys[0]])]
        elif api == 1:
            ids, offs = gv.encode_with_offsets(texts[keys[0]])
            got = [np.array(ids)]
            assert len(offs) == len(ids)
        elif api == 2:
            got = [np.array(a) for a in gv.encode_batch([texts[k] for k in keys])]
        else:
            got = [None] * len(keys)

            def sink(index, ids):
                got[index] = np.array(ids)
            gv.encode_stream([texts[k] for k in keys], sink)
        for k, ids in zip(keys, got):
            assert np.array_equal(ids, expected(k)), (i, api, k)
            if k not in fresh:
                fresh[k] = W.Vocab(vocab).encode(texts[k])
            assert np.array_equal(ids, fresh[k]), (i, api, k)
            count += 1
        if api < 2 and len(texts[keys[0]]):
            st = gv.stats()
            text = texts[keys[0]]
            if debug_build:
                assert st["reserved0"] == 1, "not the bounds-checking build"
            assert st["n_total"] == R.n_symbols(text)
            assert st["round0_sorted"] in (R.kept(text), st["n_total"]), (i, keys[0], st["round0_sorted"], R.kept(text), st["n_total"])
            assert st["round0_keys_only"] == (0 if keys[0] == "wide" else 1), (i, keys[0])
            seen.append((keys[0], st))
        i += len(keys)
    assert count == len(seq)
    return seen


def test_one_handle_many_texts():
    assert len(ORDER) * ROUNDS >= 70 > R.CODE_REUSE
    seen = run_sequence(_expected)
    # (the sequence reached the full-size keys-only path, the small plan and the 32-bit symbols)
    assert any(k == "blank" and st["hist_in_keys"] == 1 for k, st in seen)
    assert any(k == "wide" and st["symbol_bits"] > 8 for k, st in seen) or all(k != "wide" for k, _ in seen)


NO_POOL = {"WP_NO_CONTEXT_POOL": "1"}  # (a child without the pool: the first encode of a handle builds its own code)


def test_stale_blank_share_both_orders(tmp_path):
    R.run_in_child(tmp_path, "test_gpu_handle_state", "_stale_blank_share_both_orders", (), NO_POOL)


def test_cached_code_meets_other_code_points(tmp_path):
    R.run_in_child(tmp_path, "test_gpu_handle_state", "_cached_code_meets_other_code_points", (), NO_POOL)


def _stale_blank_share_both_orders():
    """The share of blanks is taken when the code is built: a blank-free text behind a blank-heavy one runs with the drop
    on and nothing to drop, a blank-heavy text behind a blank-free one with the drop off — the same ids both times."""
    vocab, _ = _vocab()
    texts = _texts()
    for first, second in (("blank", "noblank"), ("noblank", "blank")):
        gv = W.Vocab(vocab)
        for key in (first, second):
            text = texts[key]
            ids, offs = gv.encode_with_offsets(text)
            assert np.array_equal(np.array(ids), _expected(key)), (first, key)
            f_ids, f_offs = W.Vocab(vocab).encode_with_offsets(text)
            assert np.array_equal(np.array(ids), np.array(f_ids)) and np.array_equal(np.array(offs), np.array(f_offs))
            st = gv.stats()
            assert st["round0_keys_only"] == 1 and st["hist_in_keys"] == 1 and st["n_total"] == N_BIG
            if key == "noblank":   # drop on (second) or off (first): every suffix is kept either way
                assert st["round0_sorted"] == N_BIG == R.kept(text)
            elif key == first:     # the code was built from this text: its own share, the drop
                assert st["round0_sorted"] == R.kept(text) < N_BIG
                assert st["radix_pass_elems"] == N_BIG + 3 * R.kept(text)
            else:                  # the cached code of a blank-free text: no drop on a text of 1/4 blanks
                assert st["round0_sorted"] == N_BIG > R.kept(text), (st["round0_sorted"], R.kept(text))


def _cached_code_meets_other_code_points():
    """The code built from Latin words, reused on the same words in Cyrillic letters and on a text that a letter of
    frequency zero at that time dominates (its codeword is among the longest)."""
    vocab, _ = _vocab()
    texts = _texts()
    gv = W.Vocab(vocab)
    for key in ("blank", "cyrillic", "dominant", "blank"):
        assert np.array_equal(gv.encode(texts[key]), _expected(key)), key
        st = gv.stats()
        assert st["round0_keys_only"] == 1 and st["hist_in_keys"] == 1
        assert st["round0_sorted"] == R.kept(texts[key]) < st["n_total"], (key, st["round0_sorted"])  # (the first text's share: 1/4)
    lens = R.code_lengths(texts["blank"], vocab)
    assert lens[ord("я")] >= 8, lens[ord("я")]


def _pool_body(out):
    vocab_x, _ = _vocab()
    vocab_y = _pool_vocab()
    texts = _texts()
    x = W.Vocab(vocab_x)
    x.encode(texts["blank"])
    assert x.stats()["round0_sorted"] == R.kept(texts["blank"])
    del x  # (destroyed: its context is parked unless WP_NO_CONTEXT_POOL=1)
    y = W.Vocab(vocab_y)
    res = {}
    for key in ("noblank", "blank"):
        res[key] = y.encode(texts[key])
        st = y.stats()
        assert st["n_total"] == N_BIG and st["round0_keys_only"] == 1 and st["hist_in_keys"] == 1
        res["sorted_" + key] = np.array([st["round0_sorted"]])
    np.savez(out, **res)


@functools.lru_cache(maxsize=None)
def _pool_vocab():
    """another vocabulary over the same characters (every word reversed): the same size of alphabet"""
    vocab, _ = _vocab()
    return sorted({("##" + w[2:][::-1]) if w.startswith("##") and len(w) > 2 else (w if w == "[UNK]" else w[::-1]) for w in vocab})


def test_pool_hands_the_cache_to_another_vocabulary(tmp_path):
    """Handle X encodes a blank-heavy text and is destroyed; handle Y, of another vocabulary with an alphabet of the same
    size, takes X's context from the pool, code and blank share with it: a blank-free and a blank-heavy text against the
    oracle and against the same calls with WP_NO_CONTEXT_POOL=1 (child processes: the pool belongs to the process)."""
    texts = _texts()
    ov = O.Vocab(_pool_vocab())
    exp = {k: ov.encode(texts[k], threads=8) for k in ("noblank", "blank")}
    res = {}
    for mode, env in (("pool", {}), ("no_pool", NO_POOL)):
        out = tmp_path / ("pool_%s.npz" % mode)
        R.run_in_child(tmp_path, "test_gpu_handle_state", "_pool_body", (str(out),), env, timeout=600)  # (asserts: nothing follows a failed child)
        res[mode] = np.load(str(out))
        for k in ("noblank", "blank"):
            assert np.array_equal(res[mode][k], exp[k]), (mode, k)
    k_blank = R.kept(texts["blank"])
    print("round0_sorted of the blank-heavy text: pool", int(res["pool"]["sorted_blank"][0]), "no pool",
          int(res["no_pool"]["sorted_blank"][0]), "kept", k_blank, "n", N_BIG)
    for mode in res:
        assert int(res[mode]["sorted_noblank"][0]) == N_BIG
        assert int(res[mode]["sorted_blank"][0]) in (k_blank, N_BIG)
    # without the pool Y builds its code from the blank-free text: no drop behind it; with the pool it inherits X's
    # share of 1/4 and drops
    assert int(res["no_pool"]["sorted_blank"][0]) == N_BIG
    assert int(res["pool"]["sorted_blank"][0]) == k_blank


def _sequence_debug(npy_dir):
    seen = run_sequence(lambda key: np.load(os.path.join(npy_dir, key + ".npy")), debug_build=True)
    assert len(seen) > 20


def test_sequence_bounds_build(tmp_path):
    """The sequence once more in the bounds-checking build: the encode fails if any of its counters is not zero."""
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    for key in ORDER:
        np.save(str(tmp_path / (key + ".npy")), _expected(key))
    R.run_in_child(tmp_path, "test_gpu_handle_state", "_sequence_debug", (str(tmp_path),), {"WP_LIB": dbg})
