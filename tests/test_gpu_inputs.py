"""The model-inputs entry points on the GPU (wp_linear_encode_inputs and its device form) against the Python model
(tests/inputs_model.py).  The vocabulary is tiny — one-letter words — so that a document of n words has exactly n ids
and the lengths that steer truncation and windows are exact by construction; the shapes sit where the two kernels can
break (lane groups, rows per workgroup, the scan tile), not at workload size."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import inputs_model as I
import rows_model as R
import wordpiece_amd as W
from test_rows_model import random_batch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")
LETTERS = "abcdefghijklmnopqrstuvwxyz"
VOCAB = ["[UNK]", "[CLS]", "[SEP]", "[PAD]"] + list(LETTERS)  # id of a letter: 4 + its index
CLS, SEP, PAD = 1, 2, 3
NAMES = {I.LONGEST_FIRST: "longest_first", I.ONLY_FIRST: "only_first", I.ONLY_SECOND: "only_second"}
UNIT = {None: -1, "byte": 0, "char": 1}


def _doc(n, rng):
    """a document of exactly n ids"""
    return " ".join(rng.choice(LETTERS) for _ in range(n)).encode()


def _kw(spec, unit=None):
    return dict(max_len=spec.max_len, cls_id=spec.cls_id, sep_id=spec.sep_id, pad_id=spec.pad_id, truncation=NAMES[spec.truncation],
                stride=None if spec.stride < 0 else spec.stride, offsets=unit)


def _same(got, exp, spec, unit, label):
    n = len(exp["lengths"])
    assert sorted(got) == sorted(["input_ids", "token_type_ids", "lengths", "sample"] + (["offsets"] if unit else [])), label
    assert got["input_ids"].shape == (n, spec.max_len) and got["token_type_ids"].shape == (n, spec.max_len), (label, got["input_ids"].shape, n)
    assert got["lengths"].shape == (n,) and got["sample"].shape == (n,), label
    as2d = lambda rows: np.array(rows, dtype=np.int64).reshape(n, spec.max_len)
    assert np.array_equal(got["input_ids"], as2d(exp["input_ids"])), label
    assert np.array_equal(got["token_type_ids"], as2d(exp["token_type_ids"])), label
    assert got["lengths"].tolist() == exp["lengths"] and got["sample"].tolist() == exp["sample"], label
    if unit:
        assert got["offsets"].dtype == np.uint32 and got["offsets"].shape == (n, spec.max_len, 2), label
        assert np.array_equal(got["offsets"], np.array(exp["offsets"], dtype=np.int64).reshape(n, spec.max_len, 2)), label


def _stats_check(gv, exp, spec, unit, label, route=1):
    st, ist = gv.stats(), gv.inputs_stats()
    assert ist == dict(n_samples=exp["n_samples"], n_out=len(exp["lengths"]), n_cut=exp["n_cut"], n_windowed=exp["n_windowed"],
                       pairs=spec.pairs, truncation=spec.truncation, stride=spec.stride), (label, ist)
    assert st["n_rows"] == exp["n_samples"] * (2 if spec.pairs else 1) and st["rows_route"] == route, label
    assert st["offsets_unit"] == UNIT[unit] and st["rows_truncated"] == 0, label


def _check(gv, model, docs, spec, unit=None, label=None, route=1):
    """explicit rows through the host entry point against the model; -> the model's batch"""
    label = (label, spec, unit)
    exp = I.build(model, docs, spec, unit)
    text, starts = R.join_docs(docs)
    got = gv.encode_inputs(text=text, doc_offsets=starts, pairs=spec.pairs, **_kw(spec, unit))
    _same(got, exp, spec, unit, label)
    if len(text) > len(docs):  # (a call that reached the device)
        _stats_check(gv, exp, spec, unit, label, route)
    return exp


@pytest.fixture(scope="module")
def handle():
    return W.Vocab(VOCAB), R.Model(VOCAB)


@pytest.mark.gpu
def test_row_geometry(handle):
    """lane groups of 4..64 and more than one trip of the column loop, every combination of specials"""
    gv, model = handle
    rng = random.Random(1)
    n = 0
    for cls_id, sep_id in ((CLS, SEP), (CLS, None), (None, SEP), (None, None)):
        for pairs in (0, 1):
            base = I.Spec(1, cls_id, sep_id, PAD, pairs)
            sp = I.specials(base)
            for max_len in sorted({max(sp, 1), sp + 1, 4, 5, 63, 64, 65, 129}):
                if max_len < sp:
                    continue
                B = max_len - sp
                lens = [0, 1, B // 2, B, B + 1, max(B - 1, 0), 2 * B + 3]
                docs = [_doc(rng.choice(lens), rng) for _ in range(10)]
                spec = base._replace(max_len=max_len)
                _check(gv, model, docs, spec, "byte" if max_len % 2 else None, "geometry")
                n += 1
                for trunc in (I.ONLY_FIRST, I.ONLY_SECOND):
                    if (trunc == I.ONLY_SECOND and not pairs) or B < 1:
                        continue
                    for stride in sorted({-1, 0, B // 3, B - 1}):
                        _check(gv, model, docs, spec._replace(truncation=trunc, stride=stride), "char" if max_len % 2 else None, "geometry")
                        n += 1
    assert n == 360


@pytest.mark.gpu
def test_sample_counts_at_workgroup_edges(handle):
    """rows per workgroup = 256 / lanes: 64 rows at max_len 4, 4 rows at max_len 64"""
    gv, model = handle
    rng = random.Random(2)
    n = 0
    for count in (1, 3, 4, 5, 63, 64, 65, 257):
        for max_len in (4, 64):
            docs = [_doc(rng.choice((0, 1, 2, 3, 5, 70)), rng) for _ in range(2 * count)]
            _check(gv, model, docs[:count], I.Spec(max_len, CLS, SEP, PAD, 0), None, count)
            _check(gv, model, docs, I.Spec(max_len, CLS, SEP, PAD, 1), "byte", count)
            _check(gv, model, docs[:count], I.Spec(max_len, CLS, None, PAD, 0, I.ONLY_FIRST, 1), None, count)
            _check(gv, model, docs, I.Spec(max_len, None, SEP, PAD, 1, I.ONLY_SECOND, 0), "char", count)
            n += 4
    assert n == 64


@pytest.mark.gpu
def test_scan_tile_edges(handle):
    """the scan of the window counts works in tiles of 2048 samples: one-word documents around that count, and a batch
    whose output rows cross a workgroup and a scan-tile boundary in the middle of one sample's windows"""
    gv, model = handle
    rng = random.Random(3)
    spec = I.Spec(4, CLS, None, PAD, 0, I.ONLY_FIRST, 1)  # W = 3, step 2; 64 output rows per workgroup
    for count in (2047, 2048, 2049):
        docs = [_doc(1, rng) for _ in range(count)]
        exp = _check(gv, model, docs, spec, None, count)
        assert len(exp["lengths"]) == count and exp["n_windowed"] == 0
        _check(gv, model, docs, spec._replace(stride=-1), None, count)
    docs = [_doc(1, rng) for _ in range(4200)]
    for i, words in ((2046, 40), (2047, 301), (2048, 7), (4095, 150), (4096, 150), (30, 200)):
        docs[i] = _doc(words, rng)
    exp = _check(gv, model, docs, spec, "byte", "mid-sample")
    first = np.searchsorted(exp["sample"], np.arange(len(docs)))  # first output row of every sample
    for s in (2047, 4095, 4096, 30):  # a multiple of 64 rows, and the output row 2048, lie strictly inside these samples' windows
        assert any(first[s] < r < first[s + 1] - 1 for r in range(64, len(exp["sample"]), 64)), s
    assert exp["n_windowed"] == 6 and len(exp["lengths"]) > 4200 + 400
    # pairs: samples 2047 / 2048 (rows 4094 .. 4097) sit on the scan-tile boundary of 2150 samples
    docs = [_doc(1, rng) for _ in range(4300)]
    for i, words in ((4094, 40), (4095, 301), (4096, 7), (4097, 150), (20, 200)):
        docs[i] = _doc(words, rng)
    for trunc, windowed in ((I.ONLY_FIRST, 3), (I.ONLY_SECOND, 2)):  # specials 3, B = 2: the fixed side keeps one id, W = 1
        exp = _check(gv, model, docs, I.Spec(5, CLS, SEP, PAD, 1, trunc, 0), None, "mid-sample pairs")
        assert exp["n_samples"] == 2150 and exp["n_windowed"] == windowed, exp["n_windowed"]


def _edge_lengths(B):
    return sorted({max(x, 0) for x in (0, 1, B // 2 - 1, B // 2, B // 2 + 1, B - 1, B, B + 1, 3 * B)})


@pytest.mark.gpu
def test_truncation(handle):
    gv, model = handle
    rng = random.Random(4)
    n_samples = 0
    for B in (10, 11):  # even and odd
        lens = _edge_lengths(B)
        assert len(lens) == 9
        docs = [_doc(l, rng) for la in lens for lb in lens for l in (la, lb)]  # every (la, lb): both ways round
        for trunc in (I.LONGEST_FIRST, I.ONLY_FIRST, I.ONLY_SECOND):
            exp = _check(gv, model, docs, I.Spec(B + 3, CLS, SEP, PAD, 1, trunc), "byte", "truncation")
            want = [(la, lb) for la in lens for lb in lens]
            for (la, lb), length in zip(want, exp["lengths"]):  # (the model's rows are the contract's: a spot check of the rule)
                assert length == 3 + min(la + lb, B) if trunc == I.LONGEST_FIRST else length <= B + 3
            if trunc == I.LONGEST_FIRST:
                assert exp["n_cut"] == sum(1 for la, lb in want if la + lb > B), (B, exp["n_cut"])
            n_samples += len(want)
        singles = [_doc(l, rng) for l in lens]
        for trunc in (I.LONGEST_FIRST, I.ONLY_FIRST):
            exp = _check(gv, model, singles, I.Spec(B + 2, CLS, SEP, PAD, 0, trunc), "char", "truncation, single")
            assert exp["lengths"] == [2 + min(l, B) for l in lens] and exp["n_cut"] == 2
            n_samples += len(lens)
    assert n_samples == 2 * (3 * 81 + 2 * 9)


@pytest.mark.gpu
def test_windows(handle):
    gv, model = handle
    rng = random.Random(5)
    n = n_rows = 0
    B = 12
    for pairs, trunc in ((0, I.ONLY_FIRST), (1, I.ONLY_FIRST), (1, I.ONLY_SECOND)):
        for fixed in ((0,) if not pairs else (0, 3, 40)):  # the fixed side: empty, one that fits, one that is cut
            # strides 0, 1, W - 2 and W - 1 (step 1), W = B - min(fixed, B - stride - 1); a fixed side that is cut leaves
            # W = stride + 1 whatever the stride: there the step is always 1
            strides = (0, 1, B - min(fixed, B) - 2, B - min(fixed, B) - 1) if fixed < B else (0, 1, 5, B - 1)
            for stride in strides:
                W = B - min(fixed, B - stride - 1)
                step = W - stride
                assert step >= 1 and (fixed < B or (W, step) == (stride + 1, 1))
                ls = sorted({0, 1, W - 1, W, W + 1, W + step, W + step + 1, 5 * W})
                docs = []
                for l in ls:
                    win, fix = _doc(l, rng), _doc(fixed, rng)
                    docs += [win] if not pairs else [win, fix] if trunc == I.ONLY_FIRST else [fix, win]
                spec = I.Spec(B + (3 if pairs else 2), CLS, SEP, PAD, pairs, trunc, stride)
                exp = _check(gv, model, docs, spec, "byte", ("windows", fixed, W, step))
                counts = np.bincount(exp["sample"], minlength=len(ls)).tolist()
                assert counts == [1 if l <= W else 1 + -(-(l - W) // step) for l in ls], (counts, ls, W, step)
                assert exp["n_windowed"] == sum(1 for l in ls if l > W) and exp["n_cut"] == (len(ls) if fixed > B - stride - 1 else 0)
                # window 0 only: the same rows, the first of every sample
                exp0 = _check(gv, model, docs, spec._replace(stride=-1), None, "window 0")
                if stride == 0:
                    first = np.searchsorted(exp["sample"], np.arange(len(ls)))
                    assert exp0["input_ids"] == [exp["input_ids"][r] for r in first]
                assert exp0["n_windowed"] == 0 and exp0["n_cut"] == sum(1 for l in ls if l > B - min(fixed, B - 1) or fixed > B - 1)
                n += 1
                n_rows += len(exp["lengths"])
    assert n == 4 * (1 + 3 + 3) and n_rows > 600


@pytest.mark.gpu
def test_offsets_with_normalisation():
    """offsets of a window cell are the encode_rows offsets of its id; under WP_NORM_BERT_UNCASED they point into the text
    that was passed (accented, upper case), not into the normalised copy"""
    gv = W.Vocab(VOCAB, normalize=W.WP_NORM_BERT_UNCASED)
    docs = ["\u00c9 a\u0301 B \u00e7 D e", "\u00dc x", "", "\u00f1 \u00d3 p q R s t u V w", "\u00c0 b", "\u00e7 d \u00e9 F g"]
    n = 0
    for unit in ("byte", "char"):
        ids, splits, offs = gv.encode_rows(docs=docs, offsets=unit)
        assert ids.tolist()[:6] == [4 + LETTERS.index(c) for c in "eabcde"]
        raw = W.Vocab(VOCAB).encode_rows(docs=["E a B c D e"], offsets=unit)[2]
        assert not np.array_equal(offs[:6], raw)  # (U+00C9 has two bytes, a + U+0301 two code points)
        assert offs[0].tolist() == ([0, 2] if unit == "byte" else [0, 1]) and offs[1][0] == (3 if unit == "byte" else 2)
        for spec in (I.Spec(9, CLS, SEP, PAD, 1), I.Spec(7, CLS, SEP, PAD, 1, I.ONLY_FIRST, 1), I.Spec(6, CLS, None, PAD, 0, I.ONLY_FIRST, 2),
                     I.Spec(8, None, SEP, PAD, 1, I.ONLY_SECOND, 0)):
            exp = I.build_from_rows(ids.tolist(), splits.tolist(), [tuple(o) for o in offs.tolist()], spec)
            text, starts = R.join_docs(docs)
            for kw in (dict(text=text, doc_offsets=starts), dict(text=text), dict(text=text[:-1])):
                got = gv.encode_inputs(pairs=spec.pairs, **kw, **_kw(spec, unit))
                _same(got, exp, spec, unit, (spec, unit))
                _stats_check(gv, exp, spec, unit, (spec, unit))
                assert gv.stats()["normalize"] == W.WP_NORM_BERT_UNCASED
                n += 1
            live = np.arange(spec.max_len)[None, :] < got["lengths"][:, None]
            special = np.isin(got["input_ids"], (CLS, SEP)) | ~live
            assert not got["offsets"][special].any() and (got["offsets"][~special][:, 1] > got["offsets"][~special][:, 0]).all()
    assert n == 24


def _tensor_call(gv, t, off, spec, unit=None, **kw):
    return gv.encode_inputs_tensor(t, doc_offsets=off, pairs=spec.pairs, **_kw(spec, unit), **kw)


def _to_numpy(out):
    import torch
    return {k: (x.view(torch.int32).cpu().numpy().view(np.uint32) if k == "offsets" else x.cpu().numpy()) for k, x in out.items()}


@pytest.mark.gpu
def test_lines_mode_and_the_odd_row_rule(handle):
    import torch
    gv, model = handle
    rng = random.Random(6)
    docs = [_doc(rng.choice((0, 1, 4, 9)), rng) for _ in range(12)]
    docs[-1] = _doc(5, rng)  # (an empty last line has no row of its own when the text ends in its newline)
    text, starts = R.join_docs(docs)
    n = 0
    for spec in (I.Spec(8, CLS, SEP, PAD, 1), I.Spec(6, CLS, SEP, PAD, 0, I.ONLY_FIRST, 1), I.Spec(8, CLS, SEP, PAD, 1, I.ONLY_SECOND, 2)):
        for unit in (None, "char"):
            exp = I.build(model, docs, spec, unit)
            for t in (text, text[:-1]):
                _same(gv.encode_inputs(text=t, pairs=spec.pairs, **_kw(spec, unit)), exp, spec, unit, ("lines", spec))
                _stats_check(gv, exp, spec, unit, ("lines", spec))
                dt = torch.frombuffer(bytearray(t), dtype=torch.uint8).to("cuda:0")
                _same(_to_numpy(_tensor_call(gv, dt, None, spec, unit)), exp, spec, unit, ("lines, tensor", spec))
                n += 1
    assert n == 12
    # an odd number of lines: WP_ERR_ARG, and nothing written into the caller's tensors
    odd_docs = [_doc(k, rng) for k in (2, 0, 3, 1, 4)]
    odd = b"\n".join(odd_docs)
    dt = torch.frombuffer(bytearray(odd), dtype=torch.uint8).to("cuda:0")
    d_off = torch.tensor([0] + np.cumsum([len(d) + 1 for d in odd_docs]).tolist(), dtype=torch.int64, device="cuda:0")
    for spec in (I.Spec(8, CLS, SEP, PAD, 1), I.Spec(8, CLS, SEP, PAD, 1, I.ONLY_FIRST, 1)):
        own = {k: torch.full(shape, -7, dtype=torch.int32, device="cuda:0")
               for k, shape in (("input_ids", (16, 8)), ("token_type_ids", (16, 8)), ("lengths", (16,)), ("sample", (16,)), ("offsets", (16, 8, 2)))}
        for t, off in ((dt, None), (torch.frombuffer(bytearray(odd + b"\n"), dtype=torch.uint8).to("cuda:0"), None),
                       (torch.frombuffer(bytearray(odd + b"\n"), dtype=torch.uint8).to("cuda:0"), d_off)):
            with pytest.raises(W.WordPieceError, match="even number of rows"):
                _tensor_call(gv, t, off, spec, "byte", out=own)
            torch.cuda.synchronize()
            assert all(bool((x == -7).all()) for x in own.values())


@pytest.mark.gpu
def test_per_document_route():
    """vocabularies that are encoded document by document give the same batches, with rows_route == 0"""
    rng = random.Random(7)
    n = 0
    for vocab in (["a\nb", "a", "b"], ["[UNK]", "a", "b", "a", "##b", "b", "c"]):
        gv, model = W.Vocab(vocab), R.Model(vocab)
        docs = [b"a", b"b", b"", b"a b ab", b"ab a", b"b b b a a b a b", b"a\nb", b"a b"]
        for spec in (I.Spec(6, 7, 8, 9, 1), I.Spec(5, 7, 8, 9, 0, I.ONLY_FIRST, 1), I.Spec(7, 7, 8, 9, 1, I.ONLY_SECOND, 0)):
            for unit in (None, "byte", "char"):
                _check(gv, model, docs, spec, unit, "per document", route=0)
                n += 1
        text = b"a b\nb\n\nab a b a"
        exp = I.build(model, R.split_lines(text), I.Spec(6, 7, 8, 9, 1), "byte")
        _same(gv.encode_inputs(text=text, pairs=True, max_len=6, cls_id=7, sep_id=8, pad_id=9, offsets="byte"), exp, I.Spec(6, 7, 8, 9, 1), "byte", "lines")
        assert gv.stats()["rows_route"] == 0
    assert n == 18


def _own(rows, max_len, fill=-7):
    import torch
    shapes = (("input_ids", (rows, max_len)), ("token_type_ids", (rows, max_len)), ("lengths", (rows,)), ("sample", (rows,)),
              ("offsets", (rows, max_len, 2)))
    return {k: torch.full(shape, fill, dtype=torch.int32, device="cuda:0") for k, shape in shapes}


@pytest.mark.gpu
def test_device_entry_point_and_handle_state():
    import torch
    rng = random.Random(8)
    gv, model = W.Vocab(VOCAB, device=0), R.Model(VOCAB)
    docs = [_doc(rng.choice((0, 1, 2, 6, 7, 30)), rng) for _ in range(90)]
    text, starts = R.join_docs(docs)
    before = (gv.encode(text), gv.encode_rows(docs=docs, offsets="byte"), gv.encode_padded(docs=docs, max_len=8, cls_id=CLS, sep_id=SEP))
    t = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    d_off = torch.tensor(starts, dtype=torch.int64, device="cuda:0")
    n = 0
    for spec in (I.Spec(8, CLS, SEP, PAD, 1), I.Spec(8, CLS, SEP, PAD, 0, I.ONLY_FIRST, 2), I.Spec(9, CLS, SEP, PAD, 1, I.ONLY_SECOND, 0)):
        for unit in (None, "byte"):
            exp = I.build(model, docs, spec, unit)
            rows = len(exp["lengths"])
            for off in (None, d_off):
                got = _tensor_call(gv, t, off, spec, unit)  # library-made tensors (lines mode: the guess may take a second call)
                assert all(x.device == t.device for x in got.values()) and got["input_ids"].dtype == torch.int32
                _same(_to_numpy(got), exp, spec, unit, ("tensor", spec))
                _stats_check(gv, exp, spec, unit, ("tensor", spec))
                _same(_to_numpy(_tensor_call(gv, t, off, spec, unit, n_out=rows)), exp, spec, unit, ("tensor, exact n_out", spec))
                own = _own(rows + 9, spec.max_len)  # caller-owned: untouched behind n_out rows
                view = _tensor_call(gv, t, off, spec, unit, out=own)
                assert view["input_ids"].data_ptr() == own["input_ids"].data_ptr() and tuple(view["input_ids"].shape) == (rows, spec.max_len)
                _same(_to_numpy(view), exp, spec, unit, ("tensor, out=", spec))
                assert all(bool((x[rows:] == -7).all()) for k, x in own.items() if k in view)
                if not unit:
                    assert bool((own["offsets"] == -7).all())
                # too little room: WP_ERR_ARG, the needed count, nothing written
                small = _own(rows - 1, spec.max_len)
                bufs = W.Inputs(*[small[k].data_ptr() for k in ("input_ids", "token_type_ids", "lengths", "sample", "offsets")])
                cspec = W._inputs_spec(pairs=spec.pairs, **_kw(spec, unit))
                need, ns = C.c_size_t(), C.c_size_t()
                torch.cuda.synchronize()
                rc = W.lib().wp_linear_encode_inputs_device(gv._h, C.c_void_p(t.data_ptr()), len(text),
                                                            None if off is None else C.c_void_p(off.data_ptr()),
                                                            0 if off is None else len(docs), C.byref(cspec), C.byref(bufs), rows - 1,
                                                            C.byref(need), C.byref(ns))
                assert rc == 6 and need.value == rows and b"capacity_rows" in W.lib().wp_last_error(), (rc, need.value, rows)
                assert all(bool((x == -7).all()) for x in small.values())
                with pytest.raises(W.WordPieceError, match="capacity_rows"):
                    _tensor_call(gv, t, off, spec, unit, out=small)
                n += 1
    assert n == 12
    # the other calls on the same handle are what they were, and what a fresh handle gives
    fresh = W.Vocab(VOCAB, device=0)
    for h in (gv, fresh):
        assert np.array_equal(h.encode(text), before[0])
        assert h.inputs_stats()["n_out"] == -1
        assert all(np.array_equal(x, y) for x, y in zip(h.encode_rows(docs=docs, offsets="byte"), before[1]))
        assert h.inputs_stats()["n_out"] == -1
        assert all(np.array_equal(x, y) for x, y in zip(h.encode_padded(docs=docs, max_len=8, cls_id=CLS, sep_id=SEP), before[2]))
        assert h.inputs_stats()["n_out"] == -1 and h.stats()["rows_truncated"] > 0


@pytest.mark.gpu
def test_equivalences_with_the_documents_calls():
    """single sequences cut longest-first are encode_padded; the rows of an untruncated pair batch are encode_rows"""
    rng = random.Random(9)
    n = n_pairs = n_rejected = 0
    for k in range(300):
        docs, vocab = random_batch(rng)
        try:
            gv = W.Vocab(vocab)
        except W.WordPieceError as e:  # (the only skip: a vocabulary the library rejects)
            assert "Vocab word is empty" in str(e)
            n_rejected += 1
            continue
        n += 1
        for max_len, cls_id, sep_id in ((6, 1, 2), (3, None, None), (64, 1, None)):
            got = gv.encode_inputs(a=docs, max_len=max_len, cls_id=cls_id, sep_id=sep_id, pad_id=5)
            pad_ids, pad_len = gv.encode_padded(docs=docs, max_len=max_len, cls_id=cls_id, sep_id=sep_id, pad_id=5)
            assert np.array_equal(got["input_ids"], pad_ids) and np.array_equal(got["lengths"], pad_len), (k, max_len)
            assert not got["token_type_ids"].any() and got["sample"].tolist() == list(range(len(docs)))
            if docs and any(docs):
                assert gv.inputs_stats()["n_out"] == -1  # (encode_padded came last)
        if len(docs) % 2:
            docs = docs[:-1]
        ids, splits = gv.encode_rows(docs=docs)
        lens = np.diff(splits)
        max_len = int(lens.max()) * 2 + 3 if len(lens) else 3
        got = gv.encode_inputs(a=docs[0::2], b=docs[1::2], max_len=max_len, cls_id=10 ** 6, sep_id=10 ** 6 + 1, pad_id=10 ** 6 + 2)
        for s in range(len(docs) // 2):
            la, lb = int(lens[2 * s]), int(lens[2 * s + 1])
            row = got["input_ids"][s]
            assert np.array_equal(row[1:1 + la], ids[splits[2 * s]:splits[2 * s + 1]]) and row[1 + la] == 10 ** 6 + 1, (k, s)
            assert np.array_equal(row[2 + la:2 + la + lb], ids[splits[2 * s + 1]:splits[2 * s + 2]]), (k, s)
            assert got["lengths"][s] == la + lb + 3 and got["token_type_ids"][s].tolist() == [0] * (2 + la) + [1] * (lb + 1) + [0] * (max_len - la - lb - 3)
            n_pairs += 1
        if docs and any(docs):
            assert gv.inputs_stats()["n_cut"] == 0
    assert n + n_rejected == 300 and n > 250 and n_pairs > 400


def _debug_cases():
    rng = random.Random(10)
    cases = []
    for spec in (I.Spec(8, CLS, SEP, PAD, 1), I.Spec(7, CLS, SEP, PAD, 0, I.ONLY_FIRST, 2), I.Spec(9, CLS, None, PAD, 1, I.ONLY_SECOND, 1),
                 I.Spec(70, CLS, SEP, PAD, 1, I.ONLY_FIRST, -1)):
        for count in (6, 300):
            cases.append(([_doc(rng.choice((0, 1, 3, 8, 25, 90)), rng) for _ in range(count)], spec))
    return cases


def _debug_run(gv, model):
    n = 0
    for docs, spec in _debug_cases():
        for unit in (None, "byte", "char"):
            _check(gv, model, docs, spec, unit, "debug")
            n += 1
    assert n == 24


@pytest.mark.gpu
def test_arena_guard():
    gv = W.Vocab(VOCAB)
    gv.set_option(W.WP_OPT_ARENA_GUARD, 1)
    _debug_run(gv, R.Model(VOCAB))
    assert gv.stats()["guard_zones"] > 0


@pytest.mark.gpu
def test_bounds_checking_build(tmp_path):
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "inputs_dbg_run.py"
    script.write_text('''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import wordpiece_amd as W
import rows_model as R
from test_gpu_inputs import VOCAB, _debug_run
gv = W.Vocab(VOCAB)
_debug_run(gv, R.Model(VOCAB))
assert gv.stats()["reserved0"] == 1, "not the bounds-checking build"
print("INPUTS_DEBUG_OK")
''' % (os.path.dirname(PKG), HERE))
    env = dict(os.environ, WP_LIB=dbg)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "INPUTS_DEBUG_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
