"""Offsets mode on the GPU (wp_linear_encode_offsets / _device): ids and spans, both units, against the Python model
(tests/offsets_model.py) on small and medium inputs, on every path of the walk (asserted through stats()), and at full
size through vectorised checks of what include/wordpiece_amd.h promises."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import offsets_model as M
import wordpiece_amd as W
from wordpiece_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")


def _model_check(gv, text, vocab, label=""):
    """ids and offsets of both units equal the model; ids equal encode() on the same handle"""
    text = text if isinstance(text, (bytes, bytearray)) else text.encode("utf8")
    exp_ids, spans, _, starts = M.encode_spans(text, vocab)
    exp_b = M.to_bytes(spans, text, starts)
    plain = gv.encode(text)
    for unit, exp in (("byte", exp_b), ("char", spans)):
        ids, offs = gv.encode_with_offsets(text, unit=unit)
        assert ids.tolist() == exp_ids, (label, unit, text[:60])
        assert offs.shape == (len(exp_ids), 2) and offs.dtype == np.uint32
        assert [tuple(r) for r in offs.tolist()] == exp, (label, unit, text[:60])
        if text:  # (an empty text is no encode: it leaves the statistics alone, as wp_linear_encode does)
            assert gv.stats()["offsets_unit"] == (0 if unit == "byte" else 1)
    assert np.array_equal(plain, np.asarray(exp_ids, dtype=np.int32)), label


@pytest.mark.gpu
def test_golden_and_random_small_cases():
    import json
    n = 0
    for name in ("reference_tests_cpp.json", "survey_probed_cases.json"):
        with open(os.path.join(HERE, "golden", name)) as f:
            for case in json.load(f)["cases"]:
                text = bytes.fromhex(case["text_hex"])
                vocab = [bytes.fromhex(w) for w in case["vocab_hex"]]
                try:
                    gv = W.Vocab(vocab)
                except W.WordPieceError:
                    continue
                _model_check(gv, text, vocab, name)
                n += 1
    assert n > 10
    rng = random.Random(7)
    for k in range(1000):
        text, vocab = M.random_case(rng)
        _model_check(W.Vocab(vocab), text, vocab, "random %d" % k)


def _medium_cases():
    """(label, text, vocab, options, expected stats) — one per path of the walk"""
    rng = np.random.default_rng(11)
    en, en_vocab = synth.english_corpus(300_000, seed=12, vocab_size=3000)
    out = [("staged class rule", en + " zqéx \xff".encode("latin1") + "中 ▁ end".encode(), en_vocab + ["[UNK]"], {},
            {"anchor_mode": 0, "staged_emit": 1})]
    # wide words (49..2048 chars) of single-char pieces, some failing
    letters = "abcdefgh"
    words = []
    for k in range(600):
        w = "".join(rng.choice(list(letters), size=int(rng.integers(49, 2049 if k % 50 == 0 else 300))))
        words.append(w + ("z" if k % 7 == 0 else ""))
        words.append("ab")
    vocab_w = ["[UNK]"] + list(letters) + ["##" + c for c in letters] + ["##ab", "abc", "##cde"]
    out.append(("wide words", " ".join(words).encode(), vocab_w, {}, {"anchor_mode": 0, "staged_emit": 1}))
    # long words: pointer doubling, with a failing one and ordinary text around
    alnum = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789", dtype=np.uint8)
    blob = lambda n: alnum[rng.integers(0, len(alnum), n)].tobytes()
    vocab_l = en_vocab + ["##" + chr(c) for c in alnum if "##" + chr(c) not in en_vocab] + ["[UNK]"]
    text_l = en[:50_000] + b" " + blob(30_000) + b" " + en[50_000:90_000] + b" " + blob(5000) + b"_" + blob(9000) + b"Q " + en[:2000]
    out.append(("long words", text_l, vocab_l, {}, {"anchor_mode": 2, "staged_emit": 0}))
    for positive in (True, False):
        s, vocab_s = synth.random_split_case(77, 300_000, 3000, positive)
        out.append(("single word %s" % positive, s.encode() if isinstance(s, str) else s, vocab_s, {},
                    {"anchor_mode": 2, "n_anchors": 1}))
    # coverage rule on the staged walk: CJK with multi-char CJK tokens
    chars = [chr(c) for c in range(0x4E00, 0x4E00 + 300)]
    cw = ["".join(rng.choice(chars, size=int(k))) for k in rng.integers(1, 5, size=3000)]
    vocab_c = ["[UNK]"] + chars[:280] + ["##" + c for c in chars[:280]] + list(dict.fromkeys(cw[:1500]))
    text_c = "".join(cw[i] for i in rng.integers(0, len(cw), size=20000)).encode("utf8")
    out.append(("coverage rule", text_c, vocab_c, {}, {"anchor_mode": 1, "staged_emit": 1}))
    small = en[:60_000] + " a\u0001b ".encode() + en[60_000:80_000]
    out.append(("sparse emit", en[:80_000], en_vocab, {W.WP_OPT_SPARSE_EMIT: 1}, {"staged_emit": 0}))
    out.append(("cover anchors", en[:80_000], en_vocab, {W.WP_OPT_COVER_ANCHORS: 1}, {"anchor_mode": 1}))
    out.append(("vocab in S", en[:80_000], en_vocab, {W.WP_OPT_VOCAB_IN_S: 1}, {"vocab_in_s": 1}))
    out.append(("U+0001 in text", small, en_vocab + ["\u0001", "##\u0001b"], {}, {"vocab_in_s": 1}))
    out.append(("full depth", en[:80_000], en_vocab, {W.WP_OPT_FULL_DEPTH: 1}, {"full_depth": 1}))
    out.append(("duplicate lines", en[:80_000], en_vocab + en_vocab[:50], {}, {"full_depth": 1}))
    wide_alpha = [chr(c) for c in range(0x400, 0x400 + 300)]
    aw = ["".join(rng.choice(wide_alpha, size=int(k))) for k in rng.integers(1, 6, size=4000)]
    text_a = " ".join(aw[i] for i in rng.integers(0, len(aw), size=20000)).encode("utf8")
    vocab_a = ["[UNK]"] + wide_alpha[:290] + ["##" + c for c in wide_alpha[:250]] + list(dict.fromkeys(aw[:2000]))
    out.append(("alphabet > 255", text_a, vocab_a, {}, {"symbol_bits": 9}))
    return out


@pytest.mark.gpu
def test_medium_inputs_on_every_path():
    for label, text, vocab, opts, want in _medium_cases():
        gv = W.Vocab(vocab)
        for k, v in opts.items():
            gv.set_option(k, v)
        _model_check(gv, text, vocab, label)
        st = gv.stats()
        for k, v in want.items():
            assert st[k] == v, (label, k, st[k])


def _cp_starts(tb):
    return np.nonzero((tb & 0xC0) != 0x80)[0]


def _seq_len(lead):
    return np.where(lead < 0x80, 1, np.where(lead < 0xE0, 2, np.where(lead < 0xF0, 3, 4)))


def _vectorised_check(gv, text, vocab):
    """ids equal encode(); token spans hold the token's bytes; spans increasing and disjoint; uncovered bytes are
    blanks; char-unit offsets map to byte-unit offsets through the text's code-point starts"""
    tb = np.frombuffer(text, dtype=np.uint8)
    plain = gv.encode(text)
    ids, ob = gv.encode_with_offsets(text, unit="byte")
    st_b = gv.stats()
    ids_c, oc = gv.encode_with_offsets(text, unit="char")
    assert np.array_equal(ids, plain) and np.array_equal(ids_c, plain)
    b, e = ob[:, 0].astype(np.int64), ob[:, 1].astype(np.int64)
    assert (b < e).all() and (b[1:] >= e[:-1]).all() and e[-1] <= len(tb)
    # token spans: the stored word's bytes
    unk = gv.unk_id
    words = [gv.token_utf8(i) or b"" for i in range(len(vocab))]
    vlen = np.array([len(w) for w in words], dtype=np.int64)
    voff = np.concatenate([[0], np.cumsum(vlen)])[:-1]
    blob = np.frombuffer(b"".join(words) + b"\0", dtype=np.uint8)
    tok = ids != unk
    if unk == -1:
        tok &= ids >= 0
    ti, tb0, te = ids[tok].astype(np.int64), b[tok], e[tok]
    assert np.array_equal(te - tb0, vlen[ti])
    for s in range(0, len(ti), 1 << 21):
        ii, bb, ll = ti[s:s + (1 << 21)], tb0[s:s + (1 << 21)], vlen[ti[s:s + (1 << 21)]]
        first = np.repeat(np.cumsum(ll) - ll, ll)
        within = np.arange(int(ll.sum())) - first
        assert np.array_equal(tb[np.repeat(bb, ll) + within], blob[np.repeat(voff[ii], ll) + within])
    # uncovered bytes: blanks (ASCII whitespace, U+2581)
    d = np.zeros(len(tb) + 1, dtype=np.int32)
    d[b] += 1
    d[e] -= 1
    cov = np.cumsum(d)[:len(tb)] > 0
    assert np.isin(tb[~cov], np.array([9, 10, 11, 12, 13, 32, 0xE2, 0x96, 0x81], dtype=np.uint8)).all()
    # char unit -> byte unit through the code-point starts
    cs = _cp_starts(tb)
    cb, ce = oc[:, 0].astype(np.int64), oc[:, 1].astype(np.int64)
    last = cs[ce - 1]
    assert np.array_equal(cs[cb], b) and np.array_equal(last + _seq_len(tb[last]), e)
    return st_b


@pytest.mark.gpu
def test_full_size_english_100mb():
    text, vocab = synth.english_corpus(100 << 20, seed=3)
    gv = W.Vocab(vocab)
    st = _vectorised_check(gv, text, vocab)
    assert st["anchor_mode"] == 0 and st["staged_emit"] == 1 and st["offsets_unit"] == 0
    print("offsets arena B/symbol %.1f" % (st["arena_bytes"] / st["n_text"]))


@pytest.mark.gpu
def test_full_size_multilingual_64mb():
    text, vocab = synth.multilingual_corpus(64 << 20, seed=4, vocab_size=120000)
    gv = W.Vocab(vocab)
    st = _vectorised_check(gv, text, vocab)
    assert st["anchor_mode"] == 1 and st["staged_emit"] == 1 and st["symbol_bits"] > 8


@pytest.mark.gpu
def test_tensor_and_repeated_calls_agree():
    import torch
    text, vocab = synth.english_corpus(1 << 20, seed=5, vocab_size=6000)
    gv = W.Vocab(vocab, device=0)
    first = gv.encode(text)
    for unit in ("byte", "char"):
        ids, offs = gv.encode_with_offsets(text, unit=unit)
        t = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
        ti, to = gv.encode_tensor(t, offsets=True, unit=unit)
        assert ti.device == t.device and to.device == t.device and tuple(to.shape) == (len(ids), 2)
        assert np.array_equal(ti.cpu().numpy(), ids)
        assert np.array_equal(to.view(torch.int32).cpu().numpy().view(np.uint32), offs)
        vi, vo = gv.encode_tensor(t, copy=False, offsets=True, unit=unit)
        assert vo.dtype == torch.uint32 and np.array_equal(vo.view(torch.int32).cpu().numpy().view(np.uint32), offs)
    assert np.array_equal(gv.encode(text), first)  # ids-only, offsets, ids-only on one handle
    st = gv.stats()
    assert st["offsets_unit"] == -1


@pytest.mark.gpu
def test_arena_guard():
    rng = random.Random(3)
    cases = [M.random_case(rng) for _ in range(40)] + [(t, v) for label, t, v, o, w in _medium_cases()[:4]]
    for text, vocab in cases:
        gv = W.Vocab(vocab)
        gv.set_option(W.WP_OPT_ARENA_GUARD, 1)
        _model_check(gv, text, vocab, "guard")
        if len(text) > 1000:
            assert gv.stats()["guard_zones"] > 0


@pytest.mark.gpu
def test_bounds_checking_build(tmp_path):
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "offsets_dbg_run.py"
    script.write_text('''
import os, sys, random
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import wordpiece_amd as W
import offsets_model as M
from test_gpu_offsets import _medium_cases, _model_check
rng = random.Random(5)
for k in range(100):
    text, vocab = M.random_case(rng)
    _model_check(W.Vocab(vocab), text, vocab, "dbg %%d" %% k)
for label, text, vocab, opts, want in _medium_cases():
    gv = W.Vocab(vocab)
    for o, v in opts.items():
        gv.set_option(o, v)
    _model_check(gv, text, vocab, label)
    assert gv.stats()["reserved0"] == 1, "not the bounds-checking build"
print("OFFSETS_DEBUG_OK")
''' % (os.path.dirname(PKG), HERE))
    env = dict(os.environ, WP_LIB=dbg)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "OFFSETS_DEBUG_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
