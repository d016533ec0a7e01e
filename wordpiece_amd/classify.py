"""Documents scored by a fastText-style linear classifier on the device (include/wordpiece_amd_classify.h): hashed word,
character-n-gram and word-n-gram features, the average of their embedding rows, one small matrix product and a softmax:
language identification and learned quality filters between lines.filter_lines_tensor and dedup_rows_tensor.  A submodule
beside the seen rows: its functions take the Vocab handle first and go through the wrapper's shared intake and result
tables, where this module registers its layer.  A handle holds up to four models, one per slot.

    from wordpiece_amd import classify
    classify.classify_load(v, words, input, output, minn=2, maxn=4, word_ngrams=1, bucket=2_000_000)   # slot 0
    r = classify.classify_rows_tensor(v, data, row_off, keep_labels=[en], min_prob=0.65, compact=True)
    v.dedup_rows_tensor(r["data"], r["row_off"])                                                       # the kept documents

The arrays of a supervised fastText model (softmax loss, not pruned, not quantised) come out of the `fasttext` package as

    ft = fasttext.load_model("lid.176.bin"); a = ft.f.getArgs()
    classify.classify_load(v, ft.get_words(), ft.get_input_matrix(), ft.get_output_matrix(), minn=a.minn, maxn=a.maxn,
                           word_ngrams=a.wordNgrams, bucket=a.bucket)          # label j is ft.get_labels()[j]

This recipe could NOT be tried where the module was written: the package is not installed there and nothing may be
downloaded, so parity with the package is not claimed; the contract is the header, tests/classify_model.py its executable
form.
"""
import ctypes as C

import numpy as np

import wordpiece_amd as W

WP_CLASSIFY_SLOTS = 4
WP_CLASSIFY_MAX_DIM, WP_CLASSIFY_MAX_LABELS, WP_CLASSIFY_MAX_MAXN, WP_CLASSIFY_MAX_WORD_NGRAMS = 512, 65535, 6, 5
WP_CLASSIFY_WANT_LOGITS, WP_CLASSIFY_WANT_COMPACT = 1, 2
CLASSIFY_REASONS = ("no_feature", "label", "min_prob")  # the bits of "reasons"
# the sizes of the kernels that a text can straddle (csrc/classify.h): the byte tile of the token and feature passes, the
# features a lane group of the accumulation takes for every lane that reads a row, the bytes of a feature-prefix group
TILE_BYTES, UNIT_STEPS, GROUP_BYTES = 1024, 4, 64
ABI_SYMBOLS = ["wp_classify_load", "wp_classify_clear", "wp_classify_rows", "wp_classify_rows_device", "wp_get_classify_stats"]


class ClassifyModel(C.Structure):
    """wp_classify_model: the host arrays and the sizes of a model."""
    _fields_ = [("words", C.c_void_p), ("word_off", C.c_void_p), ("input", C.c_void_p), ("output", C.c_void_p), ("n_words", C.c_int64), ("bucket", C.c_int64),
                ("dim", C.c_int32), ("n_labels", C.c_int32), ("minn", C.c_int32), ("maxn", C.c_int32), ("word_ngrams", C.c_int32), ("reserved", C.c_int32)]


class ClassifySpec(C.Structure):
    """wp_classify_spec: the arguments of a classify call."""
    _fields_ = [("slot", C.c_int32), ("want", C.c_int32), ("n_keep", C.c_int32), ("pad", C.c_int32), ("keep_labels", C.c_void_p), ("min_prob", C.c_float),
                ("pad2", C.c_int32), ("reserved", C.c_int64)]


class ClassifyResult(C.Structure):
    """wp_classify_result: the arrays of a classify call (host blocks, or device memory owned by the handle)."""
    _fields_ = [("label", C.c_void_p), ("prob", C.c_void_p), ("logits", C.c_void_p), ("n_features", C.c_void_p), ("row_off", C.c_void_p), ("reasons", C.c_void_p),
                ("kept", C.c_void_p), ("data", C.c_void_p), ("n_rows", C.c_int64), ("n_labels", C.c_int64), ("n_kept", C.c_int64), ("n_elems", C.c_int64)]


class ClassifyStats(C.Structure):
    """wp_classify_stats: the last classify call on a slot and the slot's model (classify_stats(v, slot))."""
    _fields_ = [(k, C.c_int64) for k in ("n_rows", "n_kept", "n_features", "n_tokens", "n_found", "n_words", "bucket", "dim", "n_labels", "minn", "maxn",
                                         "word_ngrams")]


# the layer in the wrapper's tables (wordpiece_amd: _CORPUS_LAYERS, _RESULTS, _KINDS)
W._KINDS["f32"] = (np.float32, "<f4", "float32")
W._CORPUS_LAYERS["classify"] = ("wp_classify_rows", ClassifySpec, ClassifyResult, ClassifyStats, W._BATCH, W._BATCH)
W._RESULTS["classify"] = (("label", "i32", ("rows",), None), ("prob", "f32", ("rows",), None), ("n_features", "i64", ("rows",), None),
                          ("reasons", "u32", ("rows",), None), ("logits", "f32", ("rows", "n_labels"), "logits"), ("kept", "i32", ("n_kept",), "compact"),
                          ("data", "elem", ("n_elems",), "compact"), ("row_off", "off", ("n_kept",), "compact"))


def lib():
    """The package's library with this layer's entry points bound; a library without them is an error."""
    L = W.lib()
    missing = [s for s in ABI_SYMBOLS if not hasattr(L, s)]
    if missing:
        raise W.WordPieceError("the library has no classifier: %s missing" % ", ".join(missing))
    vp, args = C.c_void_p, [C.POINTER(ClassifySpec), C.POINTER(ClassifyResult)]
    L.wp_classify_load.argtypes = [vp, C.c_int, C.POINTER(ClassifyModel)]
    L.wp_classify_clear.argtypes = [vp, C.c_int]
    L.wp_classify_rows.argtypes = [vp] + W._BATCH + args
    L.wp_classify_rows_device.argtypes = [vp] + W._BATCH + args
    L.wp_get_classify_stats.argtypes = [vp, C.c_int, C.POINTER(ClassifyStats)]  # (the slot stands between the handle and the struct)
    return L


def classify_load(v, words, input, output, *, minn, maxn, word_ngrams, bucket, slot=0):
    """A model into slot 0..3 of the handle (wp_classify_load), replacing the one there.  words: a list of str / bytes, word
    i owning row i of input; input: float32 [len(words) + bucket, dim]; output: float32 [n_labels, dim]; minn, maxn,
    word_ngrams, bucket: the model's args.  The arrays are copied to the handle's device; the model stays until
    classify_clear or the end of the handle."""
    ws = [W._bytes(w) for w in words]
    inp, outp = np.ascontiguousarray(input, dtype=np.float32), np.ascontiguousarray(output, dtype=np.float32)
    if inp.ndim != 2 or outp.ndim != 2 or inp.shape[1] != outp.shape[1] or inp.shape[0] != len(ws) + int(bucket):
        raise W.WordPieceError("classify: input must be [len(words) + bucket, dim] and output [n_labels, dim]")
    pool, off = np.frombuffer(b"".join(ws), dtype=np.uint8), W._offsets_of([len(w) for w in ws])
    m = ClassifyModel(pool.ctypes.data if pool.size else None, off.ctypes.data, inp.ctypes.data if inp.size else None, outp.ctypes.data if outp.size else None,
                      len(ws), int(bucket), inp.shape[1], outp.shape[0], int(minn), int(maxn), int(word_ngrams), 0)
    W._check(lib().wp_classify_load(v._h, int(slot), C.byref(m)))


def classify_clear(v, slot=0):
    """Frees the model of the slot (wp_classify_clear); the statistics of the slot start again."""
    W._check(lib().wp_classify_clear(v._h, int(slot)))


def classify_stats(v, slot=0):
    """wp_classify_stats of the slot as a dict: n_rows, n_kept, n_features, n_tokens, n_found of the last call on it (n_rows
    -1: none yet); n_words, bucket, dim, n_labels, minn, maxn, word_ngrams of its model (zeros: none loaded)."""
    s = ClassifyStats()
    W._check(lib().wp_get_classify_stats(v._h, int(slot), C.byref(s)))
    return {k: getattr(s, k) for k, _ in s._fields_}


def _spec(slot, keep_labels, min_prob, logits, compact):
    """-> (the spec, the array its keep_labels points into: the caller holds it while the call runs)"""
    keep = None if keep_labels is None else np.ascontiguousarray(keep_labels, dtype=np.int32).reshape(-1)
    want = (WP_CLASSIFY_WANT_LOGITS if logits else 0) | (WP_CLASSIFY_WANT_COMPACT if compact else 0)
    held = None if keep is None else (keep if keep.size else np.zeros(1, dtype=np.int32))  # (an empty list keeps no label: the pointer is not NULL)
    return ClassifySpec(int(slot), want, 0 if keep is None else keep.size, 0, None if held is None else held.ctypes.data, float(min_prob), 0, 0), held


def classify_rows(v, data, row_off, slot=0, keep_labels=None, min_prob=0.0, logits=False, compact=False, raw=False):
    """Every document of a ragged batch of text scored by the model of the slot (wp_classify_rows).  data / row_off: the
    batch as scrub_rows takes it (row_off None: the lines of a text).
    -> {"label": np.int32 [n_rows] (the argmax, -1 without a feature), "prob": np.float32 [n_rows], "n_features": np.int64
    [n_rows], "reasons": np.uint32 [n_rows] (bit 0 no feature; else bit 1 label not in keep_labels, bit 2 prob < min_prob)};
    logits: "logits" np.float32 [n_rows, n_labels]; compact: "kept", "data", "row_off", the documents with reasons 0 back
    to back.  keep_labels None keeps every label.  raw: text comes back as np.uint8."""
    batch = W._ragged_batch("classify", data, row_off)
    if batch[0].dtype != np.uint8:
        raise W.WordPieceError("classify: data must be text (bytes, uint8)")
    lib()
    spec, held = _spec(slot, keep_labels, min_prob, logits, compact)
    return v._rows_host("classify", spec, [batch], dict(logits=logits, compact=compact), raw)


def classify_rows_tensor(v, data, row_off, slot=0, keep_labels=None, min_prob=0.0, logits=False, compact=False, copy=True):
    """classify_rows for a batch in tensors on the handle's GPU (wp_classify_rows_device): data uint8, row_off int64.
    -> a dict of tensors on that device ("reasons" as int32 bit patterns).  With compact "kept", "data" and "row_off" are
    what dedup_rows_tensor and encode_rows_tensor take.  copy=False: views of the library's buffers, valid until the next
    call on this handle."""
    batches = W._ragged_tensors("classify", v._device, [(data, row_off)], ids=False)
    lib()
    spec, held = _spec(slot, keep_labels, min_prob, logits, compact)
    return v._rows_device("classify", spec, batches, dict(logits=logits, compact=compact), copy)


def classify_docs(v, docs, **how):
    """The documents of a list (str / bytes) through classify_rows (its keywords) -> its dict, and with compact=True
    "docs": the kept documents as a list of bytes."""
    bs = [W._bytes(d) for d in docs]
    r = classify_rows(v, b"".join(bs), W._offsets_of([len(b) for b in bs]), **how)
    if how.get("compact"):
        off, flat = r["row_off"], bytes(r["data"])
        r["docs"] = [flat[off[k]:off[k + 1]] for k in range(len(r["kept"]))]
    return r
