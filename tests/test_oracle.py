"""CPU tests (no GPU): pin the oracle against the reference's own golden vectors,
the survey's recorded outputs, an independent brute-force model, and the reference's
libsais/utf8/utils: their recorded answers (tests/golden/reference_lib_outputs.json), and the
libraries themselves where oracle/_ref was built from the reference checkout."""
import ctypes as C
import hashlib
import json
import os
import random

import numpy as np
import pytest

import bruteforce
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", _load("reference_tests_cpp.json"))
def test_reference_tests_cpp_vectors(case):
    text = bytes.fromhex(case["text_hex"])
    vocab = [bytes.fromhex(w) for w in case["vocab_hex"]]
    got = O.encode(text, vocab).tolist()
    if case["expected"] is not None:
        assert got == case["expected"]
    assert got == bruteforce.encode(text, vocab)


@pytest.mark.parametrize("case", _load("survey_probed_cases.json"), ids=lambda c: c["name"])
def test_survey_probed_cases(case):
    text = bytes.fromhex(case["text_hex"])
    vocab = [bytes.fromhex(w) for w in case["vocab_hex"]]
    assert O.encode(text, vocab).tolist() == case["expected"]


def test_empty_vocab_word_throws():
    for bad in (["a", "##"], ["a", ""], [b"\xff"]):
        with pytest.raises(O.OracleError, match="Vocab word is empty"):
            O.Vocab(bad)


def _random_case(rng):
    alpha = "ab-, .c"
    nt = rng.randint(1, 8)
    vocab = set()
    while len(vocab) < nt:
        w = "".join(rng.choice(alpha) for _ in range(rng.randint(1, 4)))
        if rng.random() < 0.4:
            w = "##" + w
        if w.strip("#") == "" and w.startswith("##") and len(w) == 2:
            continue
        vocab.add(w)
    vocab = sorted(vocab)
    rng.shuffle(vocab)
    text = "".join(rng.choice(alpha) for _ in range(rng.randint(0, 24)))
    return text, vocab


def test_oracle_equals_bruteforce_random():
    rng = random.Random(1234)
    n = 0
    while n < 4000:
        text, vocab = _random_case(rng)
        try:
            exp = bruteforce.encode(text, vocab)
        except RuntimeError:
            continue
        assert O.encode(text, vocab).tolist() == exp, (text, vocab)
        n += 1


def _random_split_case(rng, text_len, parts, positive):
    """tests.cpp:99-135 randomString/randomSplit (our own generator, seeds differ)."""
    s = "".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(text_len))
    borders = {text_len}
    while len(borders) < parts:
        borders.add(rng.randint(1, text_len - 1))
    res, start = set(), 0
    for b in sorted(borders):
        if start == 0:
            res.add(s[start:b])
        res.add("##" + s[start:b])
        start = b
    vocab = sorted(res)
    if not positive:
        vocab = vocab[1:]
    return s, vocab


def test_random_split_grid_vs_bruteforce():
    rng = random.Random(17)
    for text_len in range(10, 120, 5):
        for parts in (2, 3, 5, 9, 17, 33):
            parts = min(parts, text_len)
            for positive in (True, False):
                s, vocab = _random_split_case(rng, text_len, parts, positive)
                if not vocab:
                    continue
                assert O.encode(s, vocab).tolist() == bruteforce.encode(s, vocab)


def test_builtin_sa_is_plain_lexicographic_order():
    rng = np.random.default_rng(5)
    for _ in range(200):
        n = int(rng.integers(1, 60))
        S = rng.integers(0, 4, size=n).astype(np.int32)
        sa = O.suffix_array(S, 4)
        exp = sorted(range(n), key=lambda i: S[i:].tolist())
        assert sa.tolist() == exp


# The reference's libsais / utf8.cpp / utils.cpp (oracle/_ref, built from the reference checkout when it is
# there) answered the inputs below once; tests/golden/make_reference_outputs.py recorded their answers in
# reference_lib_outputs.json.  The tests check the oracle against those recorded answers everywhere, and
# against the reference's libraries themselves where oracle/_ref exists.
REF_OUTPUTS = os.path.join(HERE, "golden", "reference_lib_outputs.json")
SA_CASES = ((1, 3), (2, 2), (1000, 3), (5000, 30), (200000, 5), (300000, 100000))
CP_RANGES = ((0, 0x3100), (0x4DB0, 0x4E10), (0x9FF0, 0xA010), (0xF8F0, 0xFB10), (0x1FFF0, 0x20010),
             (0x2A6D0, 0x2A710), (0x2B730, 0x2B830), (0x2CEA0, 0x2CEC0), (0x2F7F0, 0x2FA30))
CP_CLASSES = ("is_space", "is_punctuation", "is_spacing_char")
TOKEN_WORDS = ["##", "", "##a", "[UNK]", "[a]", "##[a]", "...", ".", "##..", "a.", "[]", "#", "###", "####",
               "[ ]", ", ", "\xff", "##\xff", "aé中", "##中", "a b", "[CLS", "CLS]"]


def _recorded(key):
    with open(REF_OUTPUTS) as f:
        return json.load(f)[key]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.int32).tobytes()).hexdigest()


def _sa_inputs():
    rng = np.random.default_rng(7)
    for n, k in SA_CASES:
        S = rng.integers(0, k, size=n).astype(np.int32)
        S[rng.integers(0, n, size=n // 7 + 1)] = 1
        yield n, k, S


def _libsais_encode_input():
    return _random_split_case(random.Random(99), 20000, 300, True)


def _decode_inputs():
    rng = random.Random(3)
    pool = [b"a", b"\xd0\xbf", b"\xe4\xb8\xad", b"\xf0\x9f\x98\x80", b"\xff", b"\xc0\x80", b"\xed\xa0\x80",
            b"\xe2\x96", b"\x80", b"\xf4\x90\x80\x80", b" ", b"\xe2\x96\x81", b"\xc3", b"\xf0\x9f", b"\x00", b"\x01"]
    return [b"".join(rng.choice(pool) for _ in range(rng.randint(0, 12))) for _ in range(3000)]


def _word_bytes(w):
    return w.encode("latin-1") if "\xff" in w else w.encode("utf8")


def ref_utils_outputs(R):
    """What the reference's utils.cpp / utf8.cpp (oracle/_ref/librefutils.so, loaded as R) answer for the inputs
    of test_decode_and_vocab_equal_reference_utils, in the form reference_lib_outputs.json records."""
    R.ref_decode_utf8.restype = C.c_size_t
    R.ref_decode_utf8.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32)]
    R.ref_token.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_int64)]
    out = {}
    for f in CP_CLASSES:
        fn = getattr(R, "ref_" + f)
        fn.argtypes = [C.c_uint32]
        out[f] = [c for lo, hi in CP_RANGES for c in range(lo, hi) if fn(c)]
    out["decode"] = []
    for b in _decode_inputs():
        buf = (C.c_uint32 * (len(b) + 1))()
        n = R.ref_decode_utf8(b, len(b), buf)
        out["decode"].append(list(buf[:n]))
    out["token"] = []
    for w in TOKEN_WORDS:
        wb = _word_bytes(w)
        buf = (C.c_uint32 * (len(wb) + 1))()
        ln = C.c_int64()
        fl = R.ref_token(wb, len(wb), buf, C.byref(ln))
        out["token"].append([fl, list(buf[:ln.value]) if fl >= 0 else None])
    return out


def test_builtin_sa_equals_reference_libsais():
    rec = _recorded("suffix_array")
    assert len(rec) == len(SA_CASES)
    live = os.path.exists(O.LIBSAIS_REF)
    for (n, k, S), r in zip(_sa_inputs(), rec):
        assert (n, k, _sha(S)) == (r["n"], r["k"], r["s_sha256"]), "input differs from the recorded one"
        O.use_libsais(False)
        a = O.suffix_array(S, k)
        assert _sha(a) == r["sa_sha256"], (n, k)
        if live:
            assert O.use_libsais(True)
            b = O.suffix_array(S, k)
            O.use_libsais(False)
            assert np.array_equal(a, b)


def test_encode_same_with_reference_libsais():
    s, vocab = _libsais_encode_input()
    rec = _recorded("encode_libsais")
    assert hashlib.sha256(("\n".join([s] + vocab)).encode()).hexdigest() == rec["input_sha256"]
    a = O.encode(s, vocab)
    assert len(a) > 0 and (len(a), _sha(a)) == (rec["n_ids"], rec["ids_sha256"])
    if os.path.exists(O.LIBSAIS_REF):
        assert O.use_libsais(True)
        b = O.encode(s, vocab)
        O.use_libsais(False)
        assert np.array_equal(a, b)


def test_decode_and_vocab_equal_reference_utils():
    rec = _recorded("utils")
    if os.path.exists(O.REFUTILS):
        assert ref_utils_outputs(C.CDLL(O.REFUTILS)) == rec
    L = O.lib()
    for f in CP_CLASSES:
        mine = getattr(L, "wpo_" + f)
        assert [c for lo, hi in CP_RANGES for c in range(lo, hi) if mine(c)] == rec[f], f
    inputs = _decode_inputs()
    assert len(inputs) == len(rec["decode"])
    for b, exp in zip(inputs, rec["decode"]):
        mine, _ = O.decode_utf8(b)
        assert mine.tolist() == exp, b
        assert mine.tolist() == bruteforce.decode(b), b
    for w, (fl, word) in zip(TOKEN_WORDS, rec["token"]):
        if fl < 0:
            with pytest.raises(O.OracleError):
                O.Vocab([_word_bytes(w)])
        else:
            v = O.Vocab([_word_bytes(w)])
            assert v.flags(0) == fl and v.word(0) == word, w


def test_mt_path_equals_sequential():
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    from wordpiece_amd import synth
    text, vocab = synth.english_corpus(3_000_000, seed=11, vocab_size=3000)
    v = O.Vocab(vocab)
    a = v.encode(text)
    b = v.encode(text, threads=4)
    assert np.array_equal(a, b) and len(a) > 100000
