"""The documents entry points on the GPU (wp_linear_encode_rows / wp_linear_encode_padded and their device forms):
rows, row splits and document-relative offsets against the Python model (tests/rows_model.py) on small and medium
inputs, on both routes and every path of the walk, and at full size through vectorised checks of the contract."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import offsets_model as M
import rows_model as R
import wordpiece_amd as W
from wordpiece_amd import synth
from test_gpu_offsets import _medium_cases
from test_rows_model import random_batch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")
UNITS = (None, "byte", "char")


def _expected_route(vocab):
    """The contract's three exceptions, from the vocabulary alone: 0 (one encode per document) when an eligible token
    holds U+000A, any token holds U+0000 / U+0001, or two eligible lines are the same token; else 1 (the joined text)"""
    toks, _ = M._vocab(vocab)
    eligible = [(pf, tuple(cps)) for pf, bad, cps in toks if not bad]
    if any(10 in cps for _, cps in eligible) or any(c <= 1 for _, _, cps in toks for c in cps):
        return 0
    return 0 if len(set(eligible)) != len(eligible) else 1


def _same(got, exp, label):
    ids, splits = got[0], got[1]
    assert ids.dtype == np.int32 and splits.dtype == np.int64, label
    assert ids.tolist() == exp[0], label
    assert splits.tolist() == exp[1], label
    if exp[2] is not None:
        assert got[2].dtype == np.uint32 and got[2].shape == (len(exp[0]), 2), label
        assert [tuple(r) for r in got[2].tolist()] == exp[2], label


def _rows_check(gv, model, docs, label, route=1, offsets=True, per_doc=True):
    """explicit rows and lines mode (with and without the final newline) equal the model in every unit; the route is
    the expected one; every row equals encode_with_offsets(document) on the same handle"""
    text, starts = R.join_docs(docs)
    modes = [("explicit", text, starts, docs)]
    modes.append(("lines", text, None, R.split_lines(text)))
    if text:
        modes.append(("lines, open end", text[:-1], None, R.split_lines(text[:-1])))
    for mode, t, off, rows in modes:
        for unit in UNITS:
            exp = R.encode_rows(model, rows, unit if offsets else None)
            if unit and not offsets:
                exp = (exp[0], exp[1], None)
            got = gv.encode_rows(text=t, doc_offsets=off, offsets=unit)
            _same(got if offsets else got[:2], exp, (label, mode, unit))
            if t and not (off is not None and len(t) == len(rows)):  # (a call that reached the device)
                st = gv.stats()
                assert st["rows_route"] == route and st["n_rows"] == len(rows), (label, mode, unit, st["rows_route"])
                assert st["offsets_unit"] == {None: -1, "byte": 0, "char": 1}[unit]
                assert st["n_ids"] == len(exp[0])
    if per_doc:
        for unit in ("byte", "char"):
            ids, splits, offs = gv.encode_rows(docs=docs, offsets=unit)
            for i, d in enumerate(docs):
                di, do = gv.encode_with_offsets(d, unit=unit)
                assert np.array_equal(ids[splits[i]:splits[i + 1]], di), (label, unit, i)
                if offsets:
                    assert np.array_equal(offs[splits[i]:splits[i + 1]], do), (label, unit, i)


@pytest.mark.gpu
def test_golden_and_random_batches():
    n = 0
    for name in ("reference_tests_cpp.json", "survey_probed_cases.json"):
        with open(os.path.join(HERE, "golden", name)) as f:
            for case in json.load(f)["cases"]:
                text = bytes.fromhex(case["text_hex"])
                vocab = [bytes.fromhex(w) for w in case["vocab_hex"]]
                try:
                    gv, model = W.Vocab(vocab), R.Model(vocab)
                except (W.WordPieceError, RuntimeError):
                    continue
                route = _expected_route(vocab)
                _rows_check(gv, model, [text, b"", text], name, route=route, offsets=not any(b"\0" in w or b"\1" in w for w in vocab))
                n += 1
    assert n > 10
    rng = random.Random(1234)
    for k in range(1000):
        docs, vocab = random_batch(rng)
        assert _expected_route(vocab) == 1
        _rows_check(W.Vocab(vocab), R.Model(vocab), docs, "random %d" % k)


@pytest.mark.gpu
def test_fallback_routes():
    rng = random.Random(99)
    # duplicate eligible lines: ids and offsets against the model
    for k in range(60):
        docs, vocab = random_batch(rng)
        vocab = vocab + vocab
        rng.shuffle(vocab)
        assert _expected_route(vocab) == 0
        _rows_check(W.Vocab(vocab), R.Model(vocab), docs, "duplicates %d" % k, route=0)
    # an eligible token with U+000A: the counter-example of the joined route, then random batches
    vocab = ["a\nb", "a", "b"]
    gv, model = W.Vocab(vocab), R.Model(vocab)
    ids, splits = gv.encode_rows(docs=["a", "b"])
    assert ids.tolist() == [1, 2] and splits.tolist() == [0, 1, 2] and gv.stats()["rows_route"] == 0
    assert gv.encode(b"a\nb\n").tolist() == [0]
    _rows_check(gv, model, [b"a", b"b", b"", b"a\nb", b"ab a"], "newline token", route=0)
    for k in range(60):
        docs, vocab = random_batch(rng)
        vocab = vocab + [b"a\nb", b"##b\n", b"\n"]
        _rows_check(W.Vocab(vocab), R.Model(vocab), docs, "newline tokens %d" % k, route=0)
    # U+0000 / U+0001 in a token: ids only (the model cannot state the span of a match that reaches into the vocabulary
    # tail of S: it would index past the text), every row against encode(document)
    for k in range(60):
        docs, vocab = random_batch(rng)
        vocab = vocab + [b"a\x01", b"##\x01", b"\x00b", b"##b\x01a"]
        docs = [d + rng.choice([b"", b"a\x01", b"b\x01", b" \x00b"]) for d in docs]
        gv = W.Vocab(vocab)
        text, starts = R.join_docs(docs)
        for t, off, rows in ((text, starts, docs), (text, None, R.split_lines(text))):
            for unit in UNITS:
                got = gv.encode_rows(text=t, doc_offsets=off, offsets=unit)
                if t and len(t) != len(rows):
                    assert gv.stats()["rows_route"] == 0
                assert len(got[1]) == len(rows) + 1 and got[1][0] == 0 and got[1][-1] == len(got[0])
                for i, d in enumerate(rows):
                    assert np.array_equal(got[0][got[1][i]:got[1][i + 1]], gv.encode(d)), ("low cp", k, unit, i)


def _with_newlines(text, rng):
    """about every 20th ASCII blank becomes a newline (same class, same length), and a final newline is added"""
    tb = np.frombuffer(text, dtype=np.uint8).copy()
    blanks = np.flatnonzero(tb == 0x20)
    tb[blanks[rng.random(len(blanks)) < 0.05]] = 0x0A
    return tb.tobytes() + b"\n"


def _medium_rows_cases():
    rng = np.random.default_rng(5)
    cases = _medium_cases()
    # (the coverage-rule and wide-alphabet cases repeat some one-character lines, which sends them document by document:
    # they are also run with distinct lines, on the joined route, where the path of the walk is asserted)
    repeats = ("coverage rule", "alphabet > 255")
    cases += [(label + ", distinct lines", text, list(dict.fromkeys(vocab)), opts, want) for label, text, vocab, opts, want in cases
              if label in repeats]
    for label, text, vocab, opts, want in cases:
        route = _expected_route(vocab)
        assert route == (0 if label in ("U+0001 in text", "duplicate lines") + repeats else 1), label
        yield label, _with_newlines(text, rng), vocab, opts, (want if route == 1 else {}), route


def _medium_check(gv, label, text, vocab, want, route):
    model = R.Model(vocab)  # (the vocabulary is parsed once per case, not per row)
    rows = R.split_lines(text)
    if label.startswith("single word"):
        assert len(rows) == 1
    starts = np.concatenate([[0], np.cumsum([len(r) + 1 for r in rows])]).astype(np.int64)
    for unit in UNITS:
        exp = R.encode_rows(model, rows, unit if label != "U+0001 in text" else None)
        for off in (None, starts):
            got = gv.encode_rows(text=text, doc_offsets=off, offsets=unit)
            _same(got, exp, (label, unit, off is None))
            st = gv.stats()
            assert st["rows_route"] == route and st["n_rows"] == len(rows), (label, st["rows_route"])
            for k, v in want.items():
                assert st[k] == v, (label, k, st[k])


@pytest.mark.gpu
def test_medium_inputs_on_every_path():
    for label, text, vocab, opts, want, route in _medium_rows_cases():
        gv = W.Vocab(vocab)
        for k, v in opts.items():
            gv.set_option(k, v)
        _medium_check(gv, label, text, vocab, want, route)


def _numpy_pack(ids, rs, max_len, cls_id, sep_id, pad_id, lo, hi):
    """rows lo..hi of the padded batch, rebuilt from the rows result"""
    head = 0 if cls_id is None else 1
    specials = head + (0 if sep_id is None else 1)
    lens = np.diff(rs)[lo:hi]
    keep = np.minimum(lens, max_len - specials)
    col = np.arange(max_len)[None, :]
    out = np.full((hi - lo, max_len), pad_id, dtype=np.int32)
    mask = (col >= head) & (col < head + keep[:, None])
    src = rs[lo:hi, None] + col - head
    out[mask] = ids[src[mask]]
    if cls_id is not None:
        out[:, 0] = cls_id
    if sep_id is not None:
        out[np.arange(hi - lo), head + keep] = sep_id
    return out, (keep + specials).astype(np.int32), int((lens > keep).sum())


def _padded_check(gv, text, ids, rs, max_len, cls_id, sep_id, pad_id=0, doc_offsets=None):
    got, lens = gv.encode_padded(text=text, doc_offsets=doc_offsets, max_len=max_len, cls_id=cls_id, sep_id=sep_id, pad_id=pad_id)
    st = gv.stats()
    n_rows = len(rs) - 1
    assert got.shape == (n_rows, max_len) and got.dtype == np.int32 and lens.shape == (n_rows,) and lens.dtype == np.int32
    cut = 0
    for lo in range(0, n_rows, 1 << 18):
        hi = min(n_rows, lo + (1 << 18))
        exp, exp_len, c = _numpy_pack(ids, rs, max_len, cls_id, sep_id, pad_id, lo, hi)
        assert np.array_equal(got[lo:hi], exp) and np.array_equal(lens[lo:hi], exp_len), (max_len, cls_id, lo)
        cut += c
    assert st["rows_truncated"] == cut and st["n_rows"] == n_rows, (st["rows_truncated"], cut)
    return cut


def _full_size_check(gv, text, vocab, oracle_line_limit):
    import oracle_lib as O
    tb = np.frombuffer(text, dtype=np.uint8)
    nl = np.flatnonzero(tb == 0x0A)
    starts = np.concatenate([[0], nl + 1, [len(tb)] if tb[-1] != 0x0A else []]).astype(np.int64)
    n_rows = len(starts) - 1
    ends = starts[1:] - 1 if tb[-1] == 0x0A else np.concatenate([starts[1:-1] - 1, [len(tb)]])
    plain = gv.encode(text)
    ids, rs, ob = gv.encode_rows(text=text, offsets="byte")
    st = gv.stats()
    assert st["rows_route"] == 1 and st["n_rows"] == n_rows and st["offsets_unit"] == 0
    assert len(rs) == n_rows + 1 and rs[0] == 0 and rs[-1] == len(ids) and (np.diff(rs) >= 0).all()
    assert np.array_equal(ids, plain)  # the rows concatenated: the joined text's ids
    row = np.repeat(np.arange(n_rows), np.diff(rs))
    wi, wo = gv.encode_with_offsets(text, unit="byte")
    assert np.array_equal(wi, plain)
    ab = ob.astype(np.int64) + starts[row][:, None]
    assert np.array_equal(ab, wo.astype(np.int64))  # rebased offsets + the line start: the whole text's offsets
    assert (ab[:, 0] >= starts[row]).all() and (ab[:, 1] <= ends[row]).all() and (ab[:, 0] < ab[:, 1]).all()
    ids_c, rs_c, oc = gv.encode_rows(text=text, offsets="char")
    assert np.array_equal(ids_c, plain) and np.array_equal(rs_c, rs)
    cps = np.flatnonzero((tb & 0xC0) != 0x80)  # (valid UTF-8: the code points' first bytes)
    wi, wc = gv.encode_with_offsets(text, unit="char")
    assert np.array_equal(oc.astype(np.int64) + np.searchsorted(cps, starts[row])[:, None], wc.astype(np.int64))
    ids_n, rs_n = gv.encode_rows(text=text)
    assert np.array_equal(ids_n, plain) and np.array_equal(rs_n, rs) and gv.stats()["offsets_unit"] == -1
    # explicit rows give the same (the text ends in a newline in both corpora)
    if tb[-1] == 0x0A:
        ids_e, rs_e, oe = gv.encode_rows(text=text, doc_offsets=starts, offsets="byte")
        assert np.array_equal(ids_e, plain) and np.array_equal(rs_e, rs) and np.array_equal(oe, ob)
    # sample lines against the CPU oracle
    ov = O.Vocab(vocab)
    short = np.flatnonzero(ends - starts[:-1] <= oracle_line_limit)
    rng = np.random.default_rng(17)
    for r in rng.choice(short, size=300, replace=False):
        line = text[starts[r]:ends[r]]
        assert np.array_equal(ids[rs[r]:rs[r + 1]], ov.encode(line) if line else np.zeros(0, np.int32)), r
    # padded batches, rebuilt from the rows result
    cuts = []
    for max_len in (16, 128):
        for cls_id, sep_id in ((101, 102), (None, None)):
            cuts.append(_padded_check(gv, text, ids, rs, max_len, cls_id, sep_id))
    assert cuts[0] > 0
    return st, n_rows


@pytest.mark.gpu
def test_full_size_english_100mb_lines():
    text, vocab = synth.english_corpus(100 << 20, seed=3)
    gv = W.Vocab(vocab)
    st, n_rows = _full_size_check(gv, text, vocab, 1 << 20)
    assert st["anchor_mode"] == 0 and st["staged_emit"] == 1
    assert 1_000_000 < n_rows < 2_500_000
    print("rows %d, arena B/symbol %.1f" % (n_rows, st["arena_bytes"] / st["n_text"]))


@pytest.mark.gpu
def test_full_size_multilingual_64mb_lines():
    text, vocab = synth.multilingual_corpus(64 << 20, seed=4, vocab_size=120000)
    gv = W.Vocab(vocab)
    # (three of the four blocks are one line of 16 MB each: the oracle, which costs time in the length of the line and of
    # the 120 k vocabulary, is asked about lines of the first block)
    st, n_rows = _full_size_check(gv, text, vocab, 4096)
    assert st["anchor_mode"] == 1 and st["staged_emit"] == 1 and st["symbol_bits"] > 8


@pytest.mark.gpu
def test_tensor_entry_points_and_handle_state():
    import torch
    text, vocab = synth.english_corpus(1 << 20, seed=5, vocab_size=6000)
    text = text if text.endswith(b"\n") else text + b"\n"
    gv = W.Vocab(vocab, device=0)
    first = gv.encode(text)
    t = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    rows = R.split_lines(text)
    starts = np.concatenate([[0], np.cumsum([len(r) + 1 for r in rows])]).astype(np.int64)
    assert starts[-1] == len(text)
    d_starts = torch.from_numpy(starts).to("cuda:0")
    for unit in UNITS:
        host = gv.encode_rows(text=text, offsets=unit)
        for off in (None, d_starts):
            for copy in (True, False):
                got = gv.encode_rows_tensor(t, doc_offsets=off, offsets=unit, copy=copy)
                assert all(x.device == t.device for x in got) and len(got) == len(host)
                assert got[0].dtype == torch.int32 and got[1].dtype == torch.int64
                assert np.array_equal(got[0].cpu().numpy(), host[0]) and np.array_equal(got[1].cpu().numpy(), host[1])
                if unit:
                    assert got[2].dtype == torch.uint32 and tuple(got[2].shape) == (len(host[0]), 2)
                    assert np.array_equal(got[2].view(torch.int32).cpu().numpy().view(np.uint32), host[2])
    # an unaligned view of the text goes through the staging copy
    t1 = torch.cat([torch.zeros(1, dtype=torch.uint8, device="cuda:0"), t])[1:]
    got = gv.encode_rows_tensor(t1, offsets="byte")
    host = gv.encode_rows(text=text, offsets="byte")
    assert np.array_equal(got[1].cpu().numpy(), host[1]) and np.array_equal(got[2].view(torch.int32).cpu().numpy().view(np.uint32), host[2])
    # padded: library-made tensors and caller-owned ones, which stay untouched behind n_rows * max_len
    n_rows = len(rows)
    for max_len, cls_id, sep_id in ((16, 101, 102), (128, None, None), (40, 101, None)):
        h_ids, h_len = gv.encode_padded(text=text, max_len=max_len, cls_id=cls_id, sep_id=sep_id, pad_id=3)
        cut = gv.stats()["rows_truncated"]
        for off in (None, d_starts):
            p_ids, p_len = gv.encode_padded_tensor(t, doc_offsets=off, max_len=max_len, cls_id=cls_id, sep_id=sep_id, pad_id=3)
            assert p_ids.dtype == torch.int32 and tuple(p_ids.shape) == (n_rows, max_len) and tuple(p_len.shape) == (n_rows,)
            assert np.array_equal(p_ids.cpu().numpy(), h_ids) and np.array_equal(p_len.cpu().numpy(), h_len)
            assert gv.stats()["rows_truncated"] == cut and gv.stats()["n_rows"] == n_rows
            own_ids = torch.full((n_rows + 64, max_len), -7, dtype=torch.int32, device="cuda:0")
            own_len = torch.full((n_rows + 64,), -7, dtype=torch.int32, device="cuda:0")
            v_ids, v_len = gv.encode_padded_tensor(t, doc_offsets=off, max_len=max_len, cls_id=cls_id, sep_id=sep_id, pad_id=3,
                                                   out=(own_ids, own_len))
            assert v_ids.data_ptr() == own_ids.data_ptr() and tuple(v_ids.shape) == (n_rows, max_len)
            assert np.array_equal(own_ids[:n_rows].cpu().numpy(), h_ids) and np.array_equal(own_len[:n_rows].cpu().numpy(), h_len)
            assert bool((own_ids[n_rows:] == -7).all()) and bool((own_len[n_rows:] == -7).all())
    # too little room: WP_ERR_ARG, the needed count, nothing written
    small_ids = torch.full((n_rows - 1, 16), -7, dtype=torch.int32, device="cuda:0")
    small_len = torch.full((n_rows - 1,), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for off, nd in ((None, 0), (d_starts, n_rows)):
        need = C.c_size_t()
        rc = W.lib().wp_linear_encode_padded_device(gv._h, C.c_void_p(t.data_ptr()), len(text),
                                                    None if off is None else C.c_void_p(off.data_ptr()), nd, 16, 101, 102, 0,
                                                    C.c_void_p(small_ids.data_ptr()), C.c_void_p(small_len.data_ptr()), n_rows - 1,
                                                    C.byref(need))
        assert rc == 6 and need.value == n_rows and b"capacity_rows" in W.lib().wp_last_error()
        assert bool((small_ids == -7).all()) and bool((small_len == -7).all())
    with pytest.raises(W.WordPieceError, match="capacity_rows"):
        gv.encode_padded_tensor(t, max_len=16, out=(small_ids, small_len))
    # bad explicit rows are found by the kernel
    bad = d_starts.clone()
    bad[5] += 1
    with pytest.raises(W.WordPieceError, match="document offsets"):
        gv.encode_rows_tensor(t, doc_offsets=bad)
    # ids-only encodes around the documents calls are what they were
    assert np.array_equal(gv.encode(text), first)
    st = gv.stats()
    assert st["n_rows"] == -1 and st["rows_route"] == -1 and st["offsets_unit"] == -1 and st["rows_truncated"] == 0


def _guard_cases():
    rng = random.Random(3)
    return [random_batch(rng) for _ in range(40)]


@pytest.mark.gpu
def test_arena_guard():
    for k, (docs, vocab) in enumerate(_guard_cases()):
        gv = W.Vocab(vocab)
        gv.set_option(W.WP_OPT_ARENA_GUARD, 1)
        _rows_check(gv, R.Model(vocab), docs, "guard %d" % k, per_doc=False)
        gv.encode_padded(docs=docs, max_len=5, cls_id=1, sep_id=2)
    for label, text, vocab, opts, want, route in _medium_rows_cases():
        gv = W.Vocab(vocab)
        gv.set_option(W.WP_OPT_ARENA_GUARD, 1)
        for k, v in opts.items():
            gv.set_option(k, v)
        _medium_check(gv, label, text, vocab, want, route)
        assert gv.stats()["guard_zones"] > 0, label


@pytest.mark.gpu
def test_bounds_checking_build(tmp_path):
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "rows_dbg_run.py"
    script.write_text('''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import wordpiece_amd as W
import rows_model as R
from test_gpu_rows import _guard_cases, _medium_rows_cases, _medium_check, _rows_check
for k, (docs, vocab) in enumerate(_guard_cases()):
    gv = W.Vocab(vocab)
    _rows_check(gv, R.Model(vocab), docs, "dbg %%d" %% k, per_doc=False)
    gv.encode_padded(docs=docs, max_len=5, cls_id=1, sep_id=2)
for label, text, vocab, opts, want, route in _medium_rows_cases():
    gv = W.Vocab(vocab)
    for o, v in opts.items():
        gv.set_option(o, v)
    _medium_check(gv, label, text, vocab, want, route)
    assert gv.stats()["reserved0"] == 1, "not the bounds-checking build"
print("ROWS_DEBUG_OK")
''' % (os.path.dirname(PKG), HERE))
    env = dict(os.environ, WP_LIB=dbg)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "ROWS_DEBUG_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
