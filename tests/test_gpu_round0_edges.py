"""GPU tests (-m gpu) of the default round 0 at the sizes, symbol codes and inputs where it changes its plan
(csrc/linear_path.h, csrc/radix_sort.h, csrc/decode.h): every case compares the default handle's ids with the CPU oracle
and with WP_OPT_SORT_BLANKS=1 and WP_OPT_INDEXED_ROUND0=1 (byte offsets too on some cases of each group) and asserts from
wp_stats the branch it was built to reach — a case that no longer reaches it fails.

  A  sizes: n around kRadixSmallN = 2^21, n and n_sorted around multiples of the sort tile, n > 2^21 >= n_sorted, n_sorted
     below and around one tile, tiles that keep nothing, n around 2^22 for the layouts that still build the rank store
  B  codes: a codeword shorter than kKeys8MinLen (generic key builder: no builder histogram, no drop), blank codewords of
     2 bits and of about kMaxCodeLen bits, blanks that only the vocabulary holds, the gate kBlankDropMinShare two symbols
     and 1/1024 of the text on either side, 255 / 256 / 257 symbols in the alphabet
  C  the adversarial kinds of tests/soak_gpu.py at 2.2 M to 5.2 M symbols, 24 seeds
  and groups A and B and six seeds of C once more in the bounds-checking build, whose sort-order counter (kSiteSortOrder)
  sees the sorted array that no debug view of the default layout shows.

Groups A and B run in one child process with WP_NO_CONTEXT_POOL=1 (and one more in the bounds-checking build): in the
test process a new handle may take a parked context with the symbol code and the blank share of an earlier test's text,
and then the branch it reaches is not the one its own text asks for (the first run of the gate cases showed exactly that).

Wall time on one MI355X, same machine and job: the -m gpu suite without this file and test_gpu_handle_state.py 388 s
(121 tests), these two files 115 s (79 tests), 30 % on top — above the quarter aimed at, with group C at its 24 seeds."""
import functools
import json
import os
import random
import traceback

import numpy as np
import pytest

import oracle_lib as O
import round0_cases as R
import wordpiece_amd as W
from round0_cases import RADIX_SMALL_N, TILE, WINDOW_STORE_N

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(os.path.abspath(W.__file__))

# ---- group A: ASCII texts, so n = len(text) + 1 and kept = non-blanks + 1 are exact ----------------------------------
K1 = RADIX_SMALL_N // TILE + 2  # the first tile counts whose texts are above kRadixSmallN even at one symbol less
K2 = K1 + 200                   # ... and one a few hundred tiles higher
N_PLACE = (K1 + 19) * TILE + TILE // 2  # about 2.2 M symbols; the last tile half full


@functools.lru_cache(maxsize=None)
def _edge_vocab():
    return R.edge_vocab(7)


def _sized(n, kept, seed, end=None):
    """n symbols, `kept` of them no blanks (terminal symbol included in both)"""
    vocab, words = _edge_vocab()
    text = R.sized_text(seed, words, n - 1, n - kept, end=end)
    assert R.n_symbols(text) == n and R.kept(text) == kept
    return text, vocab


def _eighth(n, seed, end=None):
    return _sized(n, n - (n - 1) // 8, seed, end)


def _placed(where, seed):
    vocab, words = _edge_vocab()
    dotted = [w + "." for w in words]  # (a text without one blank stays a text of words)
    length = N_PLACE - 1
    nb = length // 4
    if where == "front":
        text = R.sized_text(seed, words, nb, nb) + R.sized_text(seed, dotted, length - nb, 0)
    elif where == "behind":  # the last tiles of the dropping pass keep nothing (the very last: the terminal symbol)
        text = R.sized_text(seed, dotted, length - nb, 0) + R.sized_text(seed, words, nb, nb)
        assert nb > 8 * TILE
    elif where == "middle_tile":  # one whole tile of the first pass, on its boundary, keeps nothing
        t = (K1 + 19) // 2
        text = R.blank_fill(seed, R.sized_text(seed, words, length, length // 8), t * TILE, (t + 1) * TILE)
    else:  # "last_tile_single": the last tile holds one non-blank and the terminal symbol
        lo = (K1 + 19) * TILE
        text = bytearray(R.blank_fill(seed, R.sized_text(seed, words, length, length // 8), lo, length))
        text[lo + 1234] = ord("q")
        text = bytes(text)
    assert R.n_symbols(text) == N_PLACE
    return text, vocab


BIG_DROP = dict(keys_only=1, hist=1, drop=True)     # above kRadixSmallN, blanks common: the builder's histogram, the drop
SMALL = dict(keys_only=1, hist=0, drop=False)       # up to kRadixSmallN: the small plan sorts every suffix

CASES = {}  # name -> (builder, expected branch, compare offsets too)
for _d in (-1, 0, 1, 2):  # kRadixSmallN: plan, builder histogram and drop switch in one step
    _n = RADIX_SMALL_N + _d
    CASES["A_n_small%+d" % _d] = (functools.partial(_eighth, _n, 11 + _d), BIG_DROP if _n > RADIX_SMALL_N else SMALL, _d == 1)
for _k in (K1, K2):       # RadixCfg<Key0>::kTile: n, then n_sorted, on a tile boundary and one off it
    for _d in (-1, 0, 1):
        CASES["A_n_tile%d%+d" % (_k, _d)] = (functools.partial(_eighth, _k * TILE + _d, 20 + _d), BIG_DROP, False)
        _kept = _k * TILE + _d
        _n = _kept + _kept // 7 + 1234
        assert 1 < _n % TILE < TILE - 1
        CASES["A_kept_tile%d%+d" % (_k, _d)] = (functools.partial(_sized, _n, _kept, 30 + _d), BIG_DROP, _k == K1 and _d == 0)
for _d in (-1, 0, 1):     # a full-size plan made for n, run over a length the small plan would have taken
    CASES["A_kept_small%+d" % _d] = (functools.partial(_sized, 2 * RADIX_SMALL_N + 4321, RADIX_SMALL_N + _d, 40 + _d), BIG_DROP, False)
for _kept in (2, 64, 65, TILE - 1, TILE, TILE + 1):  # n_sorted below, on and just above one tile (kWave = 64: one wave round)
    CASES["A_kept_%d" % _kept] = (functools.partial(_sized, RADIX_SMALL_N + 3 * TILE + 17, _kept, 50), BIG_DROP, _kept == 65)
for _w in ("front", "behind", "middle_tile", "last_tile_single"):
    CASES["A_blanks_" + _w] = (functools.partial(_placed, _w, 60), BIG_DROP, _w == "behind")
CASES["A_ends_letter"] = (functools.partial(_eighth, N_PLACE, 61, "letter"), BIG_DROP, False)
CASES["A_ends_blank"] = (functools.partial(_eighth, N_PLACE, 62, "blank"), BIG_DROP, False)

# ---- group B: branches the symbol code chooses -----------------------------------------------------------------------
N_B = RADIX_SMALL_N + 2 * TILE + 5  # a little above kRadixSmallN


def _iid(seed, chars, probs, length):
    rng = np.random.default_rng(seed)
    cps = rng.choice(np.array([ord(c) for c in chars], dtype=np.uint32), size=length, p=np.array(probs) / np.sum(probs))
    return cps.astype("<u4").tobytes().decode("utf-32-le").encode("utf-8")


def _dominant(which):
    """One symbol above half of the text.  The code is alphabetic (order-preserving), so only the last symbol of the
    alphabet can take a 1-bit codeword: 'z' where nothing above it occurs, and the blank U+2581 above all ASCII."""
    vocab, _ = _edge_vocab()
    if which == "letter":
        vocab = sorted(set(vocab + ["z" * k for k in (2, 3, 5, 8, 13, 21, 40)] + ["##" + "z" * k for k in (1, 2, 4, 9, 33)]))
        text = _iid(70, "z " + R.LETTERS[:25], [60, 25] + [15 / 25] * 25, N_B - 1)
        dom = "z"
    else:
        vocab = sorted(set(vocab + [R.SPACE_TOKEN, R.SPACE_TOKEN + "ab"]))
        text = _iid(71, R.SPACE_TOKEN + " " + R.LETTERS, [60, 5] + [35 / 26] * 26, N_B - 1)
        dom = R.SPACE_TOKEN
    lens = R.code_lengths(text, vocab)
    assert lens[ord(dom)] < R.KEYS8_MIN_LEN, lens[ord(dom)]
    return text, vocab


def _blank_lengths(which):
    vocab, words = _edge_vocab()
    if which == "long":  # about 200 code points, ' ' frequent, the other blanks rare: their codewords are the longest the code gives
        extra = [chr(c) for c in range(0xC0, 0xC0 + 170) if chr(c).isalpha()]
        vocab = sorted(set(vocab + extra + ["##" + c for c in extra] + [R.SPACE_TOKEN]))
        rng = random.Random(72)
        parts = []
        size = 0
        while size < N_B:
            w = rng.choice(words) if rng.random() < 0.7 else "".join(rng.choices(extra, k=rng.randint(1, 9)))
            parts.append(w + " ")
            size += len(w) + 1
        cps = list("".join(parts)[:N_B - 1])
        for j, c in enumerate("\t\n\v\f\r" + R.SPACE_TOKEN):  # all six ASCII blanks and U+2581 in one text
            for k in range(3):
                cps[(7 * j + k + 1) * 40961] = c
        text = "".join(cps).encode("utf-8")
        lens = R.code_lengths(text, vocab)
        assert len(lens) <= 255 and len(lens) >= 200, len(lens)
        # (build_symbol_code floors every weight at 1/512 of the text, which keeps the codewords of an alphabet of up to
        # 255 symbols at 10 bits or less whatever the text: 9 bits is as near kMaxCodeLen as a blank's codeword gets here)
        rare = [lens[ord(c)] for c in "\t\v\f\r" + R.SPACE_TOKEN]
        assert lens[ord(" ")] <= 4 and min(rare) >= 6 and max(rare) >= 9 and max(lens.values()) <= R.MAX_CODE_LEN, lens
    elif which == "short":  # few symbols: a 2-bit blank
        vocab = ["[UNK]", "a", "b", "c", "##a", "##b", "##c", "ab", "abc", "##bc", "cab" * 5, "##" + "abc" * 7, "bca" * 4]
        text = _iid(73, " abc", [45, 20, 20, 15], N_B - 1)
        lens = R.code_lengths(text, vocab)
        assert lens[ord(" ")] == 2, lens
    else:  # blank code points that only the vocabulary holds: they are in the alphabet and the blank table, in no key
        vocab = sorted(set(vocab + ["\t" + w for w in words[:30]] + ["a\vb", "##\fx", "\r", R.SPACE_TOKEN + "q"]))
        text = R.sized_text(74, words, N_B - 1, (N_B - 1) // 5, blanks=" \n")
    return text, vocab


N_GATE = 1024 * (RADIX_SMALL_N // 1024 + 52)  # whole 1 KB blocks (and 16-byte units), a little above kRadixSmallN


def _gate(delta2, delta1024):
    """Texts of one length with N / 16 + 2 * delta2 + N / 1024 * delta1024 blanks: 15 letters and a blank in every 16
    bytes, two blanks more or less in the first 16 KB, one more or less in every 1 KB.  (The code's histogram is taken
    from every 16th 16-KB tile of the text, the first among them: every tile holds the share of the whole text, and
    the two extra symbols are in a counted tile, so the sampled share is on the same side of 1/16 as the whole text's.)"""
    vocab, words = _edge_vocab()
    assert R.DEC_TILE % 1024 == 0 and N_GATE // R.DEC_TILE >= 64
    body = np.frombuffer(R.sized_text(75, words, N_GATE // 16 * 15, 0), np.uint8).reshape(-1, 15)
    units = np.concatenate([body, np.full((body.shape[0], 1), 32, np.uint8)], axis=1)  # (N / 16, 16)
    if delta1024 > 0:
        units[::64, 7] = 32           # a second blank in one unit of every 1 KB
    elif delta1024 < 0:
        units[::64, 15] = ord("e")    # ... or none
    for u in (3, 5):                  # (units of the first tile that the 1-KB rule leaves alone)
        if delta2 > 0:
            units[u, 7] = 32
        elif delta2 < 0:
            units[u, 15] = ord("e")
    text = units.tobytes()
    want = N_GATE // 16 + 2 * delta2 + N_GATE // 1024 * delta1024
    assert len(text) == N_GATE and R.kept(text) == N_GATE - want + 1
    return text, vocab


def _alphabet(size):
    """The same words with `size` distinct code points in text plus vocabulary (wp_stats.alphabet): 255 is the last
    size with 8-bit symbols"""
    vocab, words = _edge_vocab()
    have = {c for w in vocab for c in w} | set(R.BLANKS)
    extra = [chr(c) for c in range(0x100, 0x100 + 400) if chr(c).isalpha()][:size - len(have)]
    assert len(have) + len(extra) == size
    vocab = sorted(set(vocab + extra))
    base = R.sized_text(76, words, N_B - 1 - len(extra), (N_B - 1) // 6).decode()
    return (base[:1000] + "".join(extra) + base[1000:]).encode("utf-8"), vocab


CASES["B_short_code_letter"] = (functools.partial(_dominant, "letter"), dict(keys_only=1, hist=0, drop=False), True)
CASES["B_short_code_blank"] = (functools.partial(_dominant, "blank"), dict(keys_only=1, hist=0, drop=False), False)
CASES["B_blank_code_long"] = (functools.partial(_blank_lengths, "long"), BIG_DROP, True)
CASES["B_blank_code_short"] = (functools.partial(_blank_lengths, "short"), BIG_DROP, False)
CASES["B_blank_vocab_only"] = (functools.partial(_blank_lengths, "vocab_only"), BIG_DROP, False)
NO_DROP = dict(keys_only=1, hist=1, drop=False)
CASES["B_gate_minus_2"] = (functools.partial(_gate, -1, 0), NO_DROP, False)
CASES["B_gate_plus_2"] = (functools.partial(_gate, 1, 0), BIG_DROP, False)
CASES["B_gate_minus_1024th"] = (functools.partial(_gate, -1, -1), NO_DROP, False)
CASES["B_gate_plus_1024th"] = (functools.partial(_gate, 1, 1), BIG_DROP, False)
CASES["B_alphabet_255"] = (functools.partial(_alphabet, 255), dict(keys_only=1, hist=1, drop=True, alphabet=255), False)
CASES["B_alphabet_256"] = (functools.partial(_alphabet, 256), dict(keys_only=0, drop=False, alphabet=256), False)
CASES["B_alphabet_257"] = (functools.partial(_alphabet, 257), dict(keys_only=0, drop=False, alphabet=257), True)


def _assert_branch(st, text, expect, name):
    expect = dict(expect)
    alphabet = expect.pop("alphabet", None)
    if alphabet is not None:
        assert st["alphabet"] == alphabet and st["symbol_bits"] == (8 if alphabet <= 255 else 9), (name, st["alphabet"])
    R.assert_branch(st, text, label=name, **expect)


@functools.lru_cache(maxsize=None)
def _expected(name):
    """the oracle's ids of a case"""
    text, vocab = CASES[name][0]()
    return O.Vocab(vocab).encode(text, threads=8)


def _run_case(name, exp, debug_build):
    build, expect, offsets = CASES[name]
    text, vocab = build()
    if debug_build:  # the default handle alone: the counters of the bounds-checking build fail the encode
        gv = W.Vocab(vocab)
        ids = gv.encode(text)
        st = gv.stats()
        assert st["reserved0"] == 1, "not the bounds-checking build"
        assert np.array_equal(ids, exp), name
    else:
        st = R.check(text, vocab, exp)
    print(name, "n", st["n_total"], "sorted", st["round0_sorted"], "kept", R.kept(text), "keys_only", st["round0_keys_only"],
          "hist_in_keys", st["hist_in_keys"], "pass elems", st["radix_pass_elems"], flush=True)
    _assert_branch(st, text, expect, name)
    if offsets:
        if debug_build:
            ids2, _ = W.Vocab(vocab).encode_with_offsets(text)
            assert np.array_equal(np.array(ids2), exp), name
        else:
            R.check(text, vocab, exp, offsets=True)


def _run_cases(npy_dir, out_json, debug_build):
    """(in a child process) every case of A and B; the outcome of each, "ok" or the failure, goes to out_json as it
    comes.  An error of the library ends the run: nothing is started on the GPU after it."""
    results = {}
    for name in sorted(CASES):
        stop = False
        try:
            _run_case(name, np.load(os.path.join(npy_dir, name + ".npy")), debug_build)
            results[name] = "ok"
        except AssertionError:
            results[name] = traceback.format_exc()[-2500:]
        except Exception:
            results[name] = traceback.format_exc()[-2500:]
            stop = True
        with open(out_json, "w") as f:
            json.dump(results, f)
        if stop:
            return
    for seed in C_DEBUG_SEEDS if debug_build else ():
        case = _c_case(seed)
        if case is None:
            continue
        text, vocab, exp = case
        gv = W.Vocab(vocab)
        ids, _ = gv.encode_with_offsets(text)
        assert gv.stats()["reserved0"] == 1 and gv.stats()["round0_keys_only"] == 1
        assert np.array_equal(np.array(ids), exp), seed


def _child_results(tmp, debug_build):
    """Groups A and B in a process of their own without the context pool: a handle of this process could take a parked
    context with the symbol code and the blank share of an earlier text (test_gpu_handle_state.py tests that), and the
    branch a case reaches must follow from its own text."""
    for name in CASES:
        np.save(str(tmp / (name + ".npy")), _expected(name))
    out = tmp / "results.json"
    env = {"WP_NO_CONTEXT_POOL": "1"}
    if debug_build:
        dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
        assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
        env["WP_LIB"] = dbg
    r = R.run_in_child(tmp, "test_gpu_round0_edges", "_run_cases", (str(tmp), str(out), debug_build), env, timeout=1500, check=False)
    results = {}
    if out.exists():
        with open(str(out)) as f:
            results = json.load(f)
    tail = "child ended with %d: %s %s" % (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    return {name: results.get(name, "not run; " + tail) for name in CASES}, (r.returncode == 0 and "CHILD_OK" in r.stdout), tail


@pytest.fixture(scope="module")
def release_results(tmp_path_factory):
    return _child_results(tmp_path_factory.mktemp("round0_edges"), False)


@pytest.mark.parametrize("name", sorted(CASES))
def test_edge_case(name, release_results):
    assert release_results[0][name] == "ok", release_results[0][name]


# ---- n around 2^22 (window_store, linear_path.h) in the layouts that still store a rank for every position ---------------
# The default layout has no rank table; WP_OPT_VOCAB_IN_S=1 (S = text . 1 . vocabulary) and WP_OPT_FULL_DEPTH=1 (the
# true suffix array, same S) reach store_ranks_round0 / window_store_kernel.

@functools.lru_cache(maxsize=None)
def _window_vocab():
    rng = random.Random(80)
    vocab, words = R.letters_vocab(rng, 300)
    stream = O.Vocab(vocab).encode_debug(b"ab")["n"] - 3  # n = text . separator . vocabulary stream
    return vocab, words, stream


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_window_store_edge_vocab_in_s(d):
    vocab, words, stream = _window_vocab()
    n = WINDOW_STORE_N + d
    text = R.sized_text(81 + d, words, n - 1 - stream, (n - 1 - stream) // 7)
    gv = W.Vocab(vocab)
    gv.set_option(W.WP_OPT_VOCAB_IN_S, 1)
    ids = gv.encode(text)
    st = gv.stats()
    assert st["n_total"] == n and st["vocab_in_s"] == 1 and st["round0_keys_only"] == 0 and st["round0_sorted"] == n, st
    assert np.array_equal(ids, O.Vocab(vocab).encode(text, threads=8))
    assert np.array_equal(ids, W.Vocab(vocab).encode(text))


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_window_store_edge_full_depth_all_stages(d):
    from test_gpu_parity import check_all_stages
    vocab, words, stream = _window_vocab()
    n = WINDOW_STORE_N + d
    text = R.sized_text(84 + d, words, n - 1 - stream, (n - 1 - stream) // 7)
    gv = W.Vocab(vocab)
    gv.set_option(W.WP_OPT_FULL_DEPTH, 1)
    gv.encode(text[:1000])
    assert gv.stats()["n_total"] == 1000 + 1 + stream and gv.stats()["full_depth"] == 1  # (so the text below makes n)
    check_all_stages(text, vocab, "n = 2^22%+d" % d)


# ---- group C: the soak run's adversarial kinds above kRadixSmallN ---------------------------------------------------------
C_SEEDS = list(range(24))  # kind seed % 5, flavour (seed // 5) % 5 (round0_cases.big_case): every kind, every flavour
C_MAX_SKIPPED = len(C_SEEDS) // 8
_c_skipped = set()


def _c_case(seed):
    """(text, vocab, expected ids), or None where the oracle refuses the vocabulary"""
    text, vocab, kind, flavour = R.big_case(seed)
    try:
        ov = O.Vocab(vocab)
    except O.OracleError:
        return None
    return text, vocab, ov.encode(text, threads=8)


@pytest.mark.parametrize("seed", C_SEEDS)
def test_adversarial_above_small_n(seed):
    case = _c_case(seed)
    if case is None:  # counted here and, without a GPU, in test_round0_cases.py (no seed is refused as the oracle stands)
        _c_skipped.add(seed)
        assert len(_c_skipped) <= C_MAX_SKIPPED, sorted(_c_skipped)
        pytest.skip("the oracle refuses this vocabulary")
    text, vocab, exp = case
    st = R.check(text, vocab, exp, offsets=seed % 6 == 0)
    n = R.n_symbols(text)
    assert st["n_total"] == n > RADIX_SMALL_N and st["round0_keys_only"] == 1, (st["n_total"], n)
    assert st["round0_sorted"] in (R.kept(text), n), (st["round0_sorted"], R.kept(text), n)
    if st["round0_sorted"] < n:
        assert st["hist_in_keys"] == 1 and st["radix_pass_elems"] == n + 3 * st["round0_sorted"]


# ---- the bounds-checking build ------------------------------------------------------------------------------------------
C_DEBUG_SEEDS = [0, 6, 12, 18, 19, 20]  # six seeds of C: every kind and every flavour once more


def test_edges_bounds_build(tmp_path):
    """Groups A and B and six seeds of C in the bounds-checking build: no out-of-range address, and the sorted array of
    round 0 ascending, free of blank keys where blanks were dropped, and the same multiset as the keys the sort had to
    keep (kSiteSortOrder) — the encode fails if any is counted."""
    results, finished, tail = _child_results(tmp_path, True)
    bad = {name: r for name, r in results.items() if r != "ok"}
    assert not bad and finished, "\n".join("%s: %s" % kv for kv in sorted(bad.items())[:4]) + tail
