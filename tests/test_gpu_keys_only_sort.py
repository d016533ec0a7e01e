"""GPU tests (-m gpu) of the keys-only round-0 sort (csrc/radix_sort.h, radix_scatter_kernel without values;
csrc/decode.h, CandSet; csrc/prune.h, long_key_set_kernel): in the default layout round 0 sorts the keys alone and the
needed groups take their members' positions from the candidate list the key builder leaves.  Ids against the oracle
and against the same vocabulary with WP_OPT_INDEXED_ROUND0=1 (the (key, index) sort), on the key-lookup cases, on a
vocabulary whose many long-token keys crowd the builder's filter, on a text whose every suffix is a candidate, and in
the bounds-checking build (which also counts candidate runs that are not as long as their group)."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import wordpiece_amd as W
from wordpiece_amd import synth
from test_gpu_key_lookup import _cases

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(os.path.abspath(W.__file__))


def _crowded_filter_case(seed, n_long=20000, n_words=30000):
    """Many distinct long-token keys (20k tokens of 9-14 letters): the builder's bitmap filter is dense enough that
    keys of the text pass it without being in the set, and the exact set has to turn them away."""
    rng = random.Random(seed)
    letters = "abcdefghijklmnopqrstuvwxyz"
    longs = {"".join(rng.choice(letters) for _ in range(rng.randint(9, 14))) for _ in range(n_long)}
    vocab = set(longs)
    for w in list(longs)[:2000]:
        vocab.add(w[:4])
    vocab.update(letters)
    vocab.update("##" + c for c in letters)
    vocab.update("##" + "".join(rng.choice(letters) for _ in range(3)) for _ in range(300))
    longs = sorted(longs)
    words = []
    for _ in range(n_words):
        r = rng.random()
        if r < 0.3:
            words.append(rng.choice(longs))
        elif r < 0.5:
            w = rng.choice(longs)
            words.append(w[: rng.randint(5, len(w))] + "".join(rng.choice(letters) for _ in range(rng.randint(0, 4))))
        else:
            words.append("".join(rng.choice(letters) for _ in range(rng.randint(1, 16))))
    return " ".join(words).encode(), sorted(vocab)


def _ids_both_ways(text, vocab):
    a = W.Vocab(vocab)
    b = W.Vocab(vocab)
    b.set_option(W.WP_OPT_INDEXED_ROUND0, 1)
    ia = a.encode(text)
    sa = a.stats()
    ib = b.encode(text)
    sb = b.stats()
    assert sb["round0_keys_only"] == 0 and sb["round0_candidates"] == -1
    return ia, sa, ib


def test_keys_only_ids_match_oracle_and_indexed_sort():
    keys_only = 0
    for text, vocab in _cases() + [_crowded_filter_case(91)]:
        exp = O.Vocab(vocab).encode(text, threads=8)
        ia, st, ib = _ids_both_ways(text, vocab)
        assert np.array_equal(ia, exp), (len(text), vocab[:5])
        assert np.array_equal(ib, exp), (len(text), vocab[:5])
        if st["round0_keys_only"]:
            keys_only += 1
            # (every suffix in a needed group is a candidate; the list holds singletons and capped groups as well)
            assert st["round0_candidates"] >= st["needed_after_round0"] >= 0
            assert st["radix_pass_bytes"] <= 9 * st["radix_pass_elems"]
        else:
            assert st["round0_candidates"] == -1
    assert keys_only >= 6, keys_only


def test_keys_only_second_encode_reuses_the_handle():
    text, vocab = _crowded_filter_case(92, n_words=8000)
    exp = O.Vocab(vocab).encode(text, threads=8)
    gv = W.Vocab(vocab)
    for _ in range(3):
        assert np.array_equal(gv.encode(text), exp)
        assert gv.stats()["round0_keys_only"] == 1


def test_every_suffix_a_candidate_and_the_needed_list_retries():
    """A periodic text whose every suffix shares its key with long tokens: the candidate list holds nearly the whole
    text, and the needed list outgrows its first room and the encode runs again — same ids as the indexed sort."""
    words = [b"ab" * 40, b"ab" * 33 + b"c", b"ba" * 25]
    rng = random.Random(77)
    text = b" ".join(rng.choice(words) for _ in range(70_000))
    vocab = ["[UNK]"] + ["ab" * k for k in (1, 2, 5, 9, 14, 20, 33, 40)] + ["##" + "ab" * k for k in (1, 3, 7, 12, 21)] + \
            ["ba" * k for k in (1, 4, 11, 25)] + ["##c", "##b", "##a", "a", "b"]
    gv = W.Vocab(vocab)
    ids = gv.encode(text)
    st = gv.stats()
    assert st["round0_keys_only"] == 1 and st["list_retries"] == 1
    assert st["round0_candidates"] > st["n_total"] // 2
    ref = W.Vocab(vocab)
    ref.set_option(W.WP_OPT_INDEXED_ROUND0, 1)
    assert np.array_equal(ids, ref.encode(text))
    assert np.array_equal(gv.encode(text), ids) and gv.stats()["list_retries"] == 0


def test_keys_only_bounds_build(tmp_path):
    """The same cases and an 8 MB English text in the bounds-checking build: no out-of-range address and no candidate
    run whose length differs from its group's (kSiteCandRun) — the encode fails if any is counted."""
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "keys_only_dbg_run.py"
    script.write_text('''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import numpy as np
import oracle_lib as O, wordpiece_amd as W
from wordpiece_amd import synth
from test_gpu_key_lookup import _cases
from test_gpu_keys_only_sort import _crowded_filter_case
cases = _cases() + [_crowded_filter_case(93), synth.english_corpus(8 << 20, seed=6, vocab_size=29000)]
ran = 0
for text, vocab in cases:
    gv = W.Vocab(vocab)
    ids = gv.encode(text)
    st = gv.stats()
    assert st["reserved0"] == 1, "not the bounds-checking build"
    ran += st["round0_keys_only"]
    assert np.array_equal(ids, O.Vocab(vocab).encode(text, threads=8))
assert ran >= 6, ran
print("KEYS_ONLY_DEBUG_OK")
''' % (os.path.dirname(PKG), HERE))
    env = dict(os.environ, WP_LIB=dbg)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "KEYS_ONLY_DEBUG_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
