"""GPU checks of the Python wrapper's own work on the corpus layers (count, dedup, neardup, overlap, repeat, quality) and
on the text forms that share its staging copy (normalize_tensor, encode_tensor): the same bytes through an unaligned
tensor of ragged length, through an aligned one and through the host form; copy=False against copy=True; every key,
dtype and shape of a call without rows; and every optional key once against the layers' Python models, in both forms,
for text and for int32 ids.  The inputs are a few bytes: what is checked is the wrapper, not the kernels."""
import numpy as np
import pytest

import dedup_model
import neardup_model
import overlap_model
import quality_model
import repeat_model
import wordpiece_amd as W

VOCAB = ["[UNK]", "ab", "c", "xy", "##b", "the", "cat"]
TEXT = b"Ab c\nxy\nAb c\n"  # 13 bytes: three short lines, the first one repeated
OFF = [0, 5, 8, 13]
REF, REF_OFF = TEXT[:5], [0, 5]
NEAR = dict(shingle=2, n_perm=8, bands=4)
RULES = {"min_text_words": 2}

_handle = []


def handle():
    if not _handle:
        _handle.append(W.Vocab(VOCAB))
    return _handle[0]


def on_gpu(data, dtype=None):
    import torch
    if isinstance(data, bytes):
        return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else torch.zeros(0, dtype=torch.uint8, device="cuda")
    return torch.tensor(np.asarray(data).tolist(), dtype=dtype or torch.int64, device="cuda")


def unaligned(t):
    """the same bytes one byte behind an aligned address"""
    import torch
    u = torch.cat([torch.zeros(1, dtype=torch.uint8, device=t.device), t])[1:]
    assert u.data_ptr() % 4 == 1
    return u


# every tensor form the fold touches, all optional keys on, each result as a dict of tensors
TENSOR_FORMS = {
    "count": lambda v, t, off, ref, roff, copy: v.count_words_tensor(t, index=True, copy=copy),
    "dedup": lambda v, t, off, ref, roff, copy: v.dedup_rows_tensor(t, off, inverse=True, compact=True, copy=copy),
    "neardup": lambda v, t, off, ref, roff, copy: v.neardup_rows_tensor(t, off, inverse=True, compact=True, signatures=True, copy=copy, **NEAR),
    "overlap": lambda v, t, off, ref, roff, copy: v.overlap_rows_tensor(t, off, ref, roff, ngram=2, mask=True, ref=True, compact=True, copy=copy),
    "repeat": lambda v, t, off, ref, roff, copy: v.repeat_rows_tensor(t, off, ngram=2, mask=True, src=True, cut=True, compact=True, copy=copy),
    "quality": lambda v, t, off, ref, roff, copy: v.quality_rows_tensor(t, off, rules=RULES, compact=True, copy=copy),
    "normalize": lambda v, t, off, ref, roff, copy: {"text": v.normalize_tensor(t, flags=W.WP_NORM_BERT_UNCASED, copy=copy)},
    "encode": lambda v, t, off, ref, roff, copy: dict(zip(("ids", "offsets"), v.encode_tensor(t, offsets=True, copy=copy))),
}
ROW_FORMS = ("dedup", "neardup", "overlap", "repeat", "quality")
ROW_CASES = [(name, elem) for name in ROW_FORMS for elem in ("u8", "i32") if (name, elem) != ("quality", "i32")]  # (quality: text only)
# the host forms of the same calls over (data, offsets, reference data, reference offsets)
HOST_FORMS = {
    "count": lambda v, d, off, ref, roff: v.count_words(d, index=True, raw=True),
    "dedup": lambda v, d, off, ref, roff: v.dedup_rows(d, off, inverse=True, compact=True),
    "neardup": lambda v, d, off, ref, roff: v.neardup_rows(d, off, inverse=True, compact=True, signatures=True, **NEAR),
    "overlap": lambda v, d, off, ref, roff: v.overlap_rows(d, off, ref, roff, ngram=2, mask=True, ref=True, compact=True),
    "repeat": lambda v, d, off, ref, roff: v.repeat_rows(d, off, ngram=2, mask=True, src=True, cut=True, compact=True),
    "quality": lambda v, d, off, ref, roff: v.quality_rows(d, off, rules=RULES, compact=True),
    "normalize": lambda v, d, off, ref, roff: {"text": v.normalize(d, flags=W.WP_NORM_BERT_UNCASED)},
    "encode": lambda v, d, off, ref, roff: dict(zip(("ids", "offsets"), v.encode_with_offsets(d))),
}


def device_values(t):
    import torch
    return (t.view(torch.int32) if t.dtype == torch.uint32 else t).cpu().numpy()


def host_values(x):
    return np.frombuffer(x, dtype=np.uint8) if isinstance(x, bytes) else np.asarray(x)


def assert_equals_host(got, host, where):
    """key by key; the documented dtype difference: what the host gives as uint32 is int32 bit patterns on the device"""
    assert list(got) == list(host), where
    for k in got:
        g, h = device_values(got[k]), host_values(host[k])
        if h.dtype == np.uint32:
            assert g.dtype == np.int32, (where, k)
            g = g.view(np.uint32)
        assert g.dtype == h.dtype and g.shape == h.shape and np.array_equal(g, h), (where, k, g, h)


def assert_same_tensors(a, b, where):
    import torch
    assert list(a) == list(b), where
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].device == b[k].device, (where, k)
        x, y = (t.view(torch.int32) if t.dtype == torch.uint32 else t for t in (a[k], b[k]))
        assert torch.equal(x, y), (where, k, a[k], b[k])


@pytest.mark.gpu
def test_unaligned_ragged_text_equals_aligned_text_and_the_host_form():
    import torch
    v = handle()
    assert len(TEXT) == 13
    off, roff = on_gpu(OFF), on_gpu(REF_OFF)
    t1, ref1 = unaligned(on_gpu(TEXT)), unaligned(on_gpu(REF))
    t16, ref8 = on_gpu(TEXT + b"   "), on_gpu(REF + b"   ")  # aligned, a multiple of 4 bytes: no staging copy
    assert t16.data_ptr() % 4 == 0 and t16.numel() % 4 == 0 and ref8.data_ptr() % 4 == 0 and ref8.numel() % 4 == 0
    for name, form in TENSOR_FORMS.items():
        got = form(v, t1, off, ref1, roff, True)
        aligned = form(v, t16, off, ref8, roff, True)  # (the row forms end at offset 13; the text forms see three blanks more)
        if name == "normalize":
            assert bytes(aligned["text"][-3:].cpu().numpy()) == b"   "
            aligned["text"] = aligned["text"][:-3]
        assert_same_tensors(got, aligned, name)
        assert_equals_host(got, HOST_FORMS[name](v, TEXT, np.array(OFF, dtype=np.int64), REF, np.array(REF_OFF, dtype=np.int64)), name)
    assert torch.equal(TENSOR_FORMS["dedup"](v, t1, off, ref1, roff, True)["first"].cpu(), torch.tensor([0, 1, 0], dtype=torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TENSOR_FORMS))
def test_views_equal_copies(name):
    v = handle()
    off, roff = on_gpu(OFF), on_gpu(REF_OFF)
    t1, ref1 = unaligned(on_gpu(TEXT)), unaligned(on_gpu(REF))
    view = TENSOR_FORMS[name](v, t1, off, ref1, roff, False)
    seen = {k: x.clone() for k, x in view.items()}  # (read before the next call on the handle)
    assert all(seen[k].dtype == view[k].dtype and seen[k].shape == view[k].shape for k in view)
    assert_same_tensors(seen, TENSOR_FORMS[name](v, t1, off, ref1, roff, True), name)


# what a call without rows returns: (key, element kind, shape); "elem" is the batch's own kind, u32 the host's uint32 that
# the device gives as int32, and text data of a host call comes back as bytes
NO_ROWS = {
    "dedup": [("first", "i32", (0,)), ("kept", "i32", (0,)), ("counts", "i64", (0,)), ("inverse", "i32", (0,)), ("data", "elem", (0,)),
              ("row_off", "i64", (1,))],
    "neardup": [("cluster", "i32", (0,)), ("kept", "i32", (0,)), ("counts", "i64", (0,)), ("inverse", "i32", (0,)), ("data", "elem", (0,)),
                ("row_off", "i64", (1,)), ("signatures", "u32", (0, 8))],
    "overlap": [("hits", "i64", (0,)), ("first_hit", "i64", (0,)), ("first_ref", "i32", (0,)), ("covered", "i64", (0,)), ("mask", "u8", (0,)),
                ("ref_hits", "i64", (0,)), ("kept", "i32", (0,)), ("data", "elem", (0,)), ("row_off", "i64", (1,))],
    "repeat": [("repeats", "i64", (0,)), ("first_repeat", "i64", (0,)), ("first_src_row", "i32", (0,)), ("first_src_pos", "i64", (0,)),
               ("covered", "i64", (0,)), ("mask", "u8", (0,)), ("src", "i64", (0,)), ("kept", "i32", (0,)), ("data", "elem", (0,)),
               ("row_off", "i64", (1,)), ("cut_data", "elem", (0,)), ("cut_off", "i64", (1,))],
    "quality": [("signals", "i64", (23, 0)), ("reasons", "u32", (0,)), ("kept", "i32", (0,)), ("data", "elem", (0,)), ("row_off", "i64", (1,))],
}
NP_KINDS = {"u8": np.uint8, "i32": np.int32, "i64": np.int64, "u32": np.uint32}


@pytest.mark.gpu
@pytest.mark.parametrize("name,elem", ROW_CASES)
def test_no_rows(name, elem):
    import torch
    v = handle()
    torch_kinds = {"u8": torch.uint8, "i32": torch.int32, "i64": torch.int64, "u32": torch.int32}
    empty, none = torch.zeros(0, dtype=torch_kinds[elem], device="cuda"), torch.tensor([0], dtype=torch.int64, device="cuda")
    for copy in (True, False):
        got = TENSOR_FORMS[name](v, empty, none, empty, none, copy)
        assert list(got) == [k for k, _, _ in NO_ROWS[name]]
        for key, kind, shape in NO_ROWS[name]:
            x = got[key]
            assert x.dtype == torch_kinds[elem if kind == "elem" else kind] and tuple(x.shape) == shape and x.is_cuda, (name, key, x)
            assert not x.numel() or x.tolist() == [0], (name, key)
    h_empty, h_none = (b"" if elem == "u8" else np.zeros(0, dtype=np.int32)), np.zeros(1, dtype=np.int64)
    host = HOST_FORMS[name](v, h_empty, h_none, h_empty, h_none)
    assert list(host) == [k for k, _, _ in NO_ROWS[name]]
    for key, kind, shape in NO_ROWS[name]:
        x = host[key]
        if kind == "elem" and elem == "u8":
            assert x == b"" and isinstance(x, bytes), (name, key)
            continue
        assert isinstance(x, np.ndarray) and x.dtype == NP_KINDS[elem if kind == "elem" else kind] and x.shape == shape, (name, key, x)
        assert not x.size or x.tolist() == [0], (name, key)


@pytest.mark.gpu
def test_count_of_no_text():
    import torch
    v = handle()
    r = v.count_words(b"", index=True)
    assert list(r) == ["words", "counts", "word_index"] and r["words"] == []
    assert r["counts"].dtype == np.int64 and r["counts"].shape == (0,) and r["word_index"].dtype == np.int32 and r["word_index"].shape == (0,)
    r = v.count_words(b"", index=True, raw=True)
    assert list(r) == ["words", "word_off", "counts", "word_index"]
    assert r["words"].dtype == np.uint8 and r["words"].shape == (0,) and r["word_off"].dtype == np.int64 and r["word_off"].tolist() == [0]
    for copy in (True, False):
        t = v.count_words_tensor(torch.zeros(0, dtype=torch.uint8, device="cuda"), index=True, copy=copy)
        assert list(t) == ["words", "word_off", "counts", "word_index"]
        assert [(x.dtype, tuple(x.shape)) for x in t.values()] == [(torch.uint8, (0,)), (torch.int64, (1,)), (torch.int64, (0,)), (torch.int32, (0,))]
        assert t["word_off"].tolist() == [0]


# ---- every optional key once, against the layers' models: a duplicate, a hit, a repeat and a rule failure in four rows ----
TEXT_ROWS = [b"the cat sat\n", b"xy\n", b"the cat sat\n", b"a dog the cat\n"]
ID_ROWS = [np.array(r, dtype=np.int32).tobytes() for r in ([1, 2, 3, 4], [9], [1, 2, 3, 4], [7, 1, 2, 3])]
BATCHES = {"u8": (TEXT_ROWS, [b"cat sat\n"], 4), "i32": (ID_ROWS, [np.array([2, 3], dtype=np.int32).tobytes()], 2)}  # rows, reference rows, ngram


def model_of(name, data, off, ref, roff, eb, ngram):
    if name == "dedup":
        return dedup_model.dedup_rows(data, off, eb, want=3)
    if name == "neardup":
        return neardup_model.neardup_rows(data, off, eb, want=7, **NEAR)
    if name == "overlap":
        return overlap_model.overlap_rows(data, off, ref, roff, eb, ngram=ngram, want=7)
    if name == "repeat":
        return repeat_model.repeat_rows(data, off, eb, ngram=ngram, utf8=eb == 1, want=15)
    return quality_model.quality(data, off, limit=quality_model.limits(**RULES), stop_words=(b"the",), dup_lines=True)


def call_of(name, v, tensor, data, off, ref, roff, ngram, copy=True):
    kw = dict(copy=copy) if tensor else {}
    if name == "dedup":
        return (v.dedup_rows_tensor if tensor else v.dedup_rows)(data, off, inverse=True, compact=True, **kw)
    if name == "neardup":
        return (v.neardup_rows_tensor if tensor else v.neardup_rows)(data, off, inverse=True, compact=True, signatures=True, **NEAR, **kw)
    if name == "overlap":
        return (v.overlap_rows_tensor if tensor else v.overlap_rows)(data, off, ref, roff, ngram=ngram, mask=True, ref=True, compact=True, **kw)
    if name == "repeat":
        return (v.repeat_rows_tensor if tensor else v.repeat_rows)(data, off, ngram=ngram, mask=True, src=True, compact=True, cut=True, **kw)
    return (v.quality_rows_tensor if tensor else v.quality_rows)(data, off, rules=RULES, stop_words=["the"], dup_lines=True, compact=True, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name,elem", ROW_CASES)
def test_every_optional_key_against_the_model(name, elem):
    import torch
    v = handle()
    rows, refs, ngram = BATCHES[elem]
    eb = 1 if elem == "u8" else 4
    data, off = dedup_model.join(rows, eb)
    ref, roff = dedup_model.join(refs, eb)
    exp = model_of(name, data, off, ref, roff, eb, ngram)
    keys = [k for k in exp if k not in ("stats", "edges")]
    assert name == "quality" or (len(set(exp["kept"])) < len(rows) and len(exp["kept"]) > 0)  # (something dropped, something kept)
    as_array = (lambda b: np.frombuffer(b, dtype=np.uint8)) if eb == 1 else (lambda b: np.frombuffer(b, dtype=np.int32))
    as_tensor = lambda b: on_gpu(b) if eb == 1 else on_gpu(np.frombuffer(b, dtype=np.int32), torch.int32)
    forms = [(False, call_of(name, v, False, data if eb == 1 else as_array(data), np.array(off, dtype=np.int64), ref if eb == 1 else as_array(ref),
                             np.array(roff, dtype=np.int64), ngram)),
             (True, call_of(name, v, True, as_tensor(data), on_gpu(off), as_tensor(ref), on_gpu(roff), ngram))]
    for tensor, got in forms:
        assert sorted(got) == sorted(keys), (name, tensor)
        for k in keys:
            g = device_values(got[k]) if tensor else got[k]
            if k in ("data", "cut_data"):
                assert (g if isinstance(g, bytes) else g.tobytes()) == exp[k], (name, tensor, k)
                assert isinstance(g, bytes) == (not tensor and eb == 1) and (isinstance(g, bytes) or g.dtype == as_array(b"").dtype)
                continue
            if k in ("signatures", "reasons"):
                assert g.dtype == (np.int32 if tensor else np.uint32), (name, tensor, k)
                g = g.view(np.uint32)
            e = np.asarray(exp[k])
            assert g.shape == e.shape and np.array_equal(g, e), (name, tensor, k, g, e)
    hit = {"dedup": ("counts", 2), "neardup": ("counts", 2), "overlap": ("hits", 1), "repeat": ("repeats", 1), "quality": ("reasons", 1)}[name]
    assert max(exp[hit[0]]) >= hit[1], "the batch exercises the layer"
