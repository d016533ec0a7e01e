"""CPU checks of the classifier layer: the header against the ctypes mirrors and the library's exports, the pinned values of
the contract through tests/classify_model.py, every argument rule before a device is needed, and the calls that need none
(an empty batch is answered without a device too, but only by a slot with a model: tests/test_gpu_classify.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import classify_model as M
import wordpiece_amd as W
from wordpiece_amd import classify as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB, ARG, TOO_LARGE = ["[UNK]", "a", "b"], 6, 2


def test_symbols_and_structs_match_the_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd_classify.h")).read()
    assert sorted(re.findall(r"\b(wp_\w+)\s*\(", hdr.split("#ifndef")[1])) == sorted(K.ABI_SYMBOLS)
    assert all(hasattr(K.lib(), name) and name not in W.ABI_SYMBOLS for name in K.ABI_SYMBOLS) and "classify_rows" not in dir(W)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd_classify.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d\\n", sizeof(wp_classify_model), offsetof(wp_classify_model, bucket),\n'
                   '         offsetof(wp_classify_model, word_ngrams), sizeof(wp_classify_spec), offsetof(wp_classify_spec, keep_labels), offsetof(wp_classify_spec, min_prob),\n'
                   '         offsetof(wp_classify_spec, reserved), sizeof(wp_classify_result), offsetof(wp_classify_result, reasons), offsetof(wp_classify_result, n_labels),\n'
                   '         sizeof(wp_classify_stats), WP_CLASSIFY_SLOTS, WP_CLASSIFY_MAX_DIM, WP_CLASSIFY_MAX_LABELS, WP_CLASSIFY_MAX_MAXN, WP_CLASSIFY_MAX_WORD_NGRAMS,\n'
                   '         WP_CLASSIFY_WANT_LOGITS | WP_CLASSIFY_WANT_COMPACT, WP_CR_MIN_PROB);\n  return 0;\n}\n')
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "sz"), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "sz")], check=True, capture_output=True, text=True).stdout.split()]
    Mo, P, T, U = K.ClassifyModel, K.ClassifySpec, K.ClassifyResult, K.ClassifyStats
    assert got == [C.sizeof(Mo), Mo.bucket.offset, Mo.word_ngrams.offset, C.sizeof(P), P.keep_labels.offset, P.min_prob.offset, P.reserved.offset, C.sizeof(T),
                   T.reasons.offset, T.n_labels.offset, C.sizeof(U), K.WP_CLASSIFY_SLOTS, K.WP_CLASSIFY_MAX_DIM, K.WP_CLASSIFY_MAX_LABELS, K.WP_CLASSIFY_MAX_MAXN,
                   K.WP_CLASSIFY_MAX_WORD_NGRAMS, K.WP_CLASSIFY_WANT_LOGITS | K.WP_CLASSIFY_WANT_COMPACT, len(K.CLASSIFY_REASONS) - 1]
    assert (C.sizeof(Mo), C.sizeof(P), C.sizeof(T), C.sizeof(U)) == (72, 40, 96, 96)


def test_pinned_values_of_the_contract():
    assert (M.H(b"a"), M.H(b"</s>"), M.H(b"\xc3\xa9")) == (3826002220, 3617362777, 1023043777)
    assert M.grams("où".encode(), 1, 3) == [g.encode() for g in ("<o", "<où", "o", "où", "où>", "ù", "ù>")]
    assert M.grams(b"ab", 2, 4) == [b"<a", b"<ab", b"<ab>", b"ab", b"ab>", b"b>"]
    assert M.word_ngrams([b"the", "où".encode(), b"</s>"], 3, 2000000) == [804974, 68723, 412471]
    assert M.tokens(b" a\x00b\tc\x0bd\x0ce\rf\ng ") == [b"a", b"b", b"c", b"d", b"e", b"f", b"g", b"</s>"] and M.tokens(b"") == [b"</s>"]
    m = M.Model([b"x", b"</s>", b"x"], np.eye(5)[:, :3], np.eye(3), 1, 1, 2, 2)
    f = m.features(b"x </s>")[0]  # the one gram is that of "x": a literal </s> has none; of two equal words the first wins
    assert f[:4] == [0, 3 + M.H(b"x") % 2, 1, 1] and len(f) == 4 + 2 and m.features(b"")[0] == [1] and m.wid[b"x"] == 0


GOOD = dict(n_words=1, bucket=2, dim=2, n_labels=2, minn=1, maxn=2, word_ngrams=1, reserved=0)
BAD_MODELS = [(dict(dim=0), ARG, b"dim"), (dict(dim=513), ARG, b"dim"), (dict(n_labels=0), ARG, b"n_labels"), (dict(n_labels=65536), ARG, b"n_labels"),
              (dict(maxn=7), ARG, b"maxn"), (dict(minn=3), ARG, b"minn"), (dict(minn=0), ARG, b"minn"), (dict(word_ngrams=0), ARG, b"word_ngrams"),
              (dict(word_ngrams=6), ARG, b"word_ngrams"), (dict(bucket=0), ARG, b"bucket"), (dict(bucket=0, minn=0, maxn=0, word_ngrams=2), ARG, b"bucket"),
              (dict(bucket=-1), ARG, b"bucket"), (dict(n_words=-1), ARG, b"n_words"), (dict(reserved=1), ARG, b"reserved"), (dict(bucket=2 ** 31), TOO_LARGE, b"n_words + bucket"),
              (dict(input=None), ARG, b"input is NULL"), (dict(output=None), ARG, b"output is NULL"), (dict(word_off=None), ARG, b"word_off is NULL"),
              (dict(words=None), ARG, b"words is NULL"), (dict(off=(0, 2, 1), n_words=2), ARG, b"word 1"), (dict(off=(1, 2)), ARG, b"word 0"), (dict(slot=4), ARG, b"slot"),
              (dict(slot=-1), ARG, b"slot"), (dict(model=None), ARG, b"m is NULL")]


@pytest.mark.parametrize("fields,code,msg", BAD_MODELS, ids=["%s" % (f,) for f, _, _ in BAD_MODELS])
def test_model_errors_come_before_the_device_and_name_the_field(fields, code, msg):
    v, f = W.Vocab(VOCAB), dict(fields)
    pool, off, mat = np.frombuffer(b"ab", dtype=np.uint8), np.asarray(f.pop("off", (0, 2)), dtype=np.int64), np.zeros((3, 2), dtype=np.float32)
    ptr = dict(words=pool.ctypes.data, word_off=off.ctypes.data, input=mat.ctypes.data, output=mat.ctypes.data)
    ptr.update((k, f.pop(k)) for k in list(f) if k in ptr)
    slot, has_model = f.pop("slot", 0), f.pop("model", True)
    m = K.ClassifyModel(ptr["words"], ptr["word_off"], ptr["input"], ptr["output"], **dict(GOOD, **f))
    assert K.lib().wp_classify_load(v._h, slot, C.byref(m) if has_model else None) == code
    err = K.lib().wp_last_error()
    assert msg in err and err.startswith(b"classify: "), err
    assert K.classify_stats(v)["dim"] == 0  # nothing was loaded


def _call(v, spec, device, out=True, data=b"abab", off=(0, 2, 4), n=None):
    """one of the two calls with a result full of garbage (the call clears it) -> (code, result)"""
    o = K.ClassifyResult(*range(1, 13))
    sp, op = None if spec is None else C.byref(spec), C.byref(o) if out else None
    off = None if off is None else np.asarray(off, dtype=np.int64)
    n = (0 if off is None else len(off) - 1) if n is None else n
    if device:  # (pointers that are never dereferenced: the argument rules come first)
        return K.lib().wp_classify_rows_device(v._h, C.c_void_p(256), None if off is None else C.c_void_p(512), n, sp, op), o
    return K.lib().wp_classify_rows(v._h, data, None if off is None else off.ctypes.data, n, sp, op), o


BAD_CALLS = [(dict(spec=None), ARG, b"spec is NULL"), (dict(out=False), ARG, b"out is NULL"), (dict(slot=4), ARG, b"slot"), (dict(slot=-1), ARG, b"slot"),
             (dict(want=4), ARG, b"want has bits outside 3"), (dict(pad=1), ARG, b"pad must be 0"), (dict(pad2=1), ARG, b"pad2"), (dict(reserved=1), ARG, b"reserved"),
             (dict(n_keep=-1), ARG, b"n_keep"), (dict(n_keep=1), ARG, b"keep_labels is NULL"), (dict(min_prob=1.5), ARG, b"min_prob"), (dict(min_prob=-0.5), ARG, b"min_prob"),
             (dict(min_prob=float("nan")), ARG, b"min_prob"), (dict(off=None, n=2), ARG, b"row_off is NULL"), (dict(n=2 ** 31), TOO_LARGE, b"2^31 rows or more"),
             (dict(slot=1), ARG, b"slot 1 holds no model")]
HOST_ONLY = [(dict(data=None), ARG, b"data is NULL"), (dict(off=(0, 3, 2)), ARG, b"row 1"), (dict(off=(1, 2)), ARG, b"row 0"), (dict(off=(0, 2 ** 32)), TOO_LARGE, b"UINT32_MAX")]


@pytest.mark.parametrize("fields,code,msg", BAD_CALLS + HOST_ONLY, ids=["%s" % (f,) for f, _, _ in BAD_CALLS + HOST_ONLY])
def test_call_errors_come_before_the_device_and_name_the_field(fields, code, msg):
    """(a keep label outside the model needs a model, and a model a device: tests/test_gpu_classify.py)"""
    v, f = W.Vocab(VOCAB), dict(fields)
    how = {k: f.pop(k) for k in list(f) if k in ("out", "data", "off", "n")}
    spec = None if "spec" in f else K.ClassifySpec(0, 0, 0, 0, None, 0.0, 0, 0)
    for name, x in ({} if spec is None else f).items():
        setattr(spec, name, x)
    for device in ((False,) if (fields, code, msg) in HOST_ONLY else (False, True)):
        rc, o = _call(v, spec, device, **how)
        err = K.lib().wp_last_error()
        assert rc == code and msg in err and err.startswith(b"classify: "), (device, err)
        assert not how.get("out", True) or not any(getattr(o, k) for k, _ in o._fields_), device
    assert K.classify_stats(v)["n_rows"] == -1  # none of these was a call


def test_what_needs_no_device():
    v = W.Vocab(VOCAB)
    assert K.classify_stats(v, 3) == dict(dict.fromkeys([k for k, _ in K.ClassifyStats._fields_], 0), n_rows=-1)
    K.classify_clear(v, 2)  # (an empty slot: nothing to free)
    with pytest.raises(W.WordPieceError, match="slot 0 holds no model"):
        K.classify_rows(v, b"", [0])  # (an empty batch is answered without a device, but only by a model, and a model needs one)
    with pytest.raises(W.WordPieceError, match=r"input must be \[len\(words\) \+ bucket, dim\]"):
        K.classify_load(v, ["a"], np.zeros((2, 2)), np.zeros((2, 3)), minn=0, maxn=0, word_ngrams=1, bucket=1)
    assert K.lib().wp_get_classify_stats(v._h, 4, C.byref(K.ClassifyStats())) == ARG and b"classify: slot" in K.lib().wp_last_error()
