"""GPU tests (-m gpu) of the walk's key-space step lookup (csrc/scanline.h, "the step table in key space"; walk.h,
step_value): in the default layout a position's step value comes from its round-0 key, and rank[] is read only for
the keys of needed groups.  Ids against the oracle on texts built to reach every branch of that lookup, in the
default layout and with the vocabulary in S (which keeps the slot-space lookup), and in the bounds-checking build,
which also counts step starts that would break the key-space table."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import wordpiece_amd as W
from wordpiece_amd import synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(os.path.abspath(W.__file__))


def _shared_prefix_case(seed, n_words=4000, n_stems=40):
    """Long tokens that share their first 8+ characters (one round-0 key, a needed group), with shorter tokens that
    are prefixes of them and continuations that run past the group's end in the sorted order."""
    rng = np.random.default_rng(seed)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))
    stems = ["".join(rng.choice(letters, int(rng.integers(9, 14)))) for _ in range(n_stems)]
    vocab = set()
    for st in stems:
        for cut in (3, 5, len(st)):
            vocab.add(st[:cut])
        for _ in range(4):  # long tokens inside the stem's group
            vocab.add(st + "".join(rng.choice(letters, int(rng.integers(1, 8)))))
    for c in letters:
        vocab.add(c)
        vocab.add("##" + c)
    for _ in range(60):
        vocab.add("##" + "".join(rng.choice(letters, int(rng.integers(2, 6)))))
    vocab = sorted(vocab)
    words = []
    for _ in range(n_words):
        st = stems[int(rng.integers(0, n_stems))]
        kind = int(rng.integers(0, 4))
        if kind == 0:
            words.append(st)
        elif kind == 1:
            words.append(st + "".join(rng.choice(letters, int(rng.integers(1, 10)))))
        elif kind == 2:
            words.append(st[: int(rng.integers(1, len(st)))])
        else:
            words.append("".join(rng.choice(letters, int(rng.integers(1, 12)))))
    return " ".join(words).encode(), vocab


def _cases():
    cases = [_shared_prefix_case(s) for s in (1, 2, 3)]
    # a long token whose key occurs at a single suffix of the text (no tied group to refine)
    cases.append((b"qwertyuiopasdfgh zz qwerty", ["qwertyuiopasdfgh", "qwerty", "z", "##z", "q", "##w"]))
    # needed keys at the top of the key range: runs of the highest symbol, long tokens made of it
    cases.append((("z" * 70 + " ") * 30 + "z" * 41 + " azz z",
                  ["z" * 40, "z" * 12, "z" * 3, "z", "##z", "##" + "z" * 20, "a", "##zz"]))
    cases.append(((("ÿ" * 50 + " ") * 20 + "ÿ").encode(), ["ÿ" * 33, "ÿ", "##ÿ"]))
    # almost every lookup lands in a needed group (config-5-like deep shared prefixes)
    cases.append(synth.deep_prefix_corpus(600_000, seed=81))
    # both index sizes: a small text (one index) and one large enough for the coarse index of its own
    cases.append(synth.english_corpus(30_000, seed=82, vocab_size=3000))
    cases.append(synth.english_corpus(3_000_000, seed=83, vocab_size=29000))
    # random splits: every piece is a token, keys cut through the middle of them
    cases.append(synth.random_split_case(84, 4000, 300))
    return [(t if isinstance(t, (bytes, bytearray)) else t.encode(), v) for t, v in cases]


@pytest.mark.parametrize("vocab_in_s", [0, 1])
def test_key_lookup_ids_match_oracle(vocab_in_s):
    key_path = 0
    for text, vocab in _cases():
        exp = O.Vocab(vocab).encode(text, threads=8)
        gv = W.Vocab(vocab)
        if vocab_in_s:
            gv.set_option(W.WP_OPT_VOCAB_IN_S, 1)
        for _ in range(2):  # (second call: reused context, cached symbol code, remembered list size)
            got = gv.encode(text)
            assert np.array_equal(got, exp), (len(text), vocab[:5])
        st = gv.stats()
        if vocab_in_s:
            assert st["vocab_in_s"] == 1
        key_path += st["vocab_in_s"] == 0 and st["trie_refine"] == 1
    # (the default layout gives way to the reference's for some vocabularies; most cases take the key-space lookup)
    assert vocab_in_s or key_path >= 6, key_path


def test_key_lookup_bounds_build(tmp_path):
    """The same cases and the 16 MB English text in the bounds-checking build: no out-of-range address, and no step
    start strictly inside a run of equal keys that is not a needed group and changes the value (kSiteKeyStep)."""
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "key_dbg_run.py"
    script.write_text('''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import numpy as np
import oracle_lib as O, wordpiece_amd as W
from wordpiece_amd import synth
from test_gpu_key_lookup import _cases
cases = _cases() + [synth.english_corpus(16 << 20, seed=5, vocab_size=29000)]
for text, vocab in cases:
    gv = W.Vocab(vocab)
    ids = gv.encode(text)
    st = gv.stats()
    assert st["reserved0"] == 1, "not the bounds-checking build"
    assert np.array_equal(ids, O.Vocab(vocab).encode(text, threads=8))
print("KEY_DEBUG_OK")
''' % (os.path.dirname(PKG), HERE))
    env = dict(os.environ, WP_LIB=dbg)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "KEY_DEBUG_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
