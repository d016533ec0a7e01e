"""The repetition signals of a document (include/wordpiece_amd_repetition.h): its most frequent word 2-, 3- and 4-gram
and its duplicated word 5- to 10-grams, with the nine rules over them, on the device and exactly.  A submodule beside the
quality calls of the package: its functions take the Vocab handle first and go through the wrapper's shared intake and
result tables, where this module registers its layer.

    from wordpiece_amd import repetition
    r = repetition.repetition_rows_tensor(v, data, row_off, rules="gopher", compact=True)
    v.dedup_rows_tensor(r["data"], r["row_off"])
"""
import ctypes as C

import numpy as np

import wordpiece_amd as W

WP_RPT_WANT_COMPACT = 1
# the signals and the rules of a repetition call, by index (WP_RPT_*; rule k is about the n-grams of k + 2 words)
REPETITION_SIGNALS = ("words", "word_chars", "top_2_count", "top_2_chars", "top_3_count", "top_3_chars", "top_4_count", "top_4_chars",
                      "dup_5_chars", "dup_6_chars", "dup_7_chars", "dup_8_chars", "dup_9_chars", "dup_10_chars")
REPETITION_RULES = ("max_top_2_chars", "max_top_3_chars", "max_top_4_chars", "max_dup_5_chars", "max_dup_6_chars", "max_dup_7_chars",
                    "max_dup_8_chars", "max_dup_9_chars", "max_dup_10_chars")
ABI_SYMBOLS = ["wp_repetition_rows", "wp_repetition_rows_device", "wp_get_repetition_stats"]
_PRESETS = {
    # the thresholds of the MassiveText (Gopher) repetition filters, in thousandths
    "gopher": dict(zip(REPETITION_RULES, (200, 180, 160, 150, 140, 130, 120, 110, 100))),
}


def repetition_rules(name):
    """The rules of a published pipeline as the `rules` of the repetition calls: "gopher".  They are the paper's limits
    over THIS library's words and over WORD_CHARS as the denominator: parity with DataTrove's tokeniser, its greedy
    non-overlapping scan of the duplicated n-grams and its len(text) denominator is not claimed."""
    if name not in _PRESETS:
        raise W.WordPieceError("repetition: no such preset: %r (known: %s)" % (name, ", ".join(sorted(_PRESETS))))
    return dict(_PRESETS[name])


class RepetitionSpec(C.Structure):
    """wp_repetition_spec: the arguments of a repetition call (want: WP_RPT_WANT_*; limit: -1 or the threshold of rule k)."""
    _fields_ = [("elem_bytes", C.c_int32), ("want", C.c_int32), ("limit", C.c_int64 * 9), ("reserved", C.c_int64)]


class RepetitionResult(C.Structure):
    """wp_repetition_result: the arrays of a repetition call (host blocks, or device memory owned by the handle)."""
    _fields_ = [("signals", C.c_void_p), ("row_off", C.c_void_p), ("reasons", C.c_void_p), ("kept", C.c_void_p), ("data", C.c_void_p),
                ("n_rows", C.c_int64), ("n_kept", C.c_int64), ("n_elems", C.c_int64)]


class RepetitionStats(C.Structure):
    """wp_repetition_stats: the statistics of the last repetition call (repetition_stats(v))."""
    _fields_ = [("n_rows", C.c_int64), ("n_bytes", C.c_int64), ("n_words", C.c_int64), ("n_word_chars", C.c_int64), ("n_kept", C.c_int64),
                ("rule_failed", C.c_int64 * 9)]


# the layer in the wrapper's tables (wordpiece_amd: _CORPUS_LAYERS, _RESULTS)
W._CORPUS_LAYERS["repetition"] = ("wp_repetition_rows", RepetitionSpec, RepetitionResult, RepetitionStats, W._BATCH, W._BATCH)
W._RESULTS["repetition"] = (("signals", "i64", ("n_signals", "rows"), None), ("reasons", "u32", ("rows",), None), ("kept", "i32", ("n_kept",), "compact"),
                            ("data", "elem", ("n_elems",), "compact"), ("row_off", "off", ("n_kept",), "compact"))


def lib():
    """The package's library with this layer's entry points bound (the package binds them itself where it loads the
    library after this module registered the layer); a library without them is an error."""
    L = W.lib()
    missing = [s for s in ABI_SYMBOLS if not hasattr(L, s)]
    if missing:
        raise W.WordPieceError("the library has no repetition layer: %s missing" % ", ".join(missing))
    if L.wp_repetition_rows.argtypes is None:
        vp, args = C.c_void_p, [C.POINTER(RepetitionSpec), C.POINTER(RepetitionResult)]
        L.wp_repetition_rows.argtypes = [vp] + W._BATCH + args
        L.wp_repetition_rows_device.argtypes = [vp] + W._BATCH + args
        L.wp_get_repetition_stats.argtypes = [vp, C.POINTER(RepetitionStats)]
    return L


def _spec(rules, compact):
    rules = repetition_rules(rules) if isinstance(rules, str) else dict(rules or {})
    limit = [-1] * len(REPETITION_RULES)
    for name, value in rules.items():
        if name not in REPETITION_RULES:
            raise W.WordPieceError("repetition: no such rule: %r" % (name,))
        limit[REPETITION_RULES.index(name)] = int(value)
    return RepetitionSpec(1, WP_RPT_WANT_COMPACT if compact else 0, (C.c_int64 * 9)(*limit), 0)


def repetition_stats(v):
    """wp_repetition_stats of the last repetition call on v as a dict (n_rows -1: no such call yet; rule_failed: a list by rule)."""
    lib()
    return v._stats(RepetitionStats, "wp_get_repetition_stats")


def repetition_rows(v, data, row_off, rules=None, compact=False, raw=False):
    """The repetition signals of every row of a ragged batch of text and the rules over them (wp_repetition_rows).  data /
    row_off: the batch as quality_rows takes it (offsets None: the lines of a text).  rules: {name of REPETITION_RULES:
    limit in thousandths of WORD_CHARS} or the name of a preset.  -> {"signals": np.int64 [14, n_rows] (rows of
    REPETITION_SIGNALS), "reasons": np.uint32 [n_rows] (bit k: rule k failed)}, with compact "kept": np.int32 (the rows
    that failed no rule) and their "data" and "row_off" back to back.  raw: the data comes back as np.uint8."""
    batch = W._ragged_batch("repetition", data, row_off)
    if batch[0].dtype != np.uint8:
        raise W.WordPieceError("repetition: data must be text")
    lib()
    return v._rows_host("repetition", _spec(rules, compact), [batch], dict(compact=compact), raw, n_signals=len(REPETITION_SIGNALS))


def repetition_rows_tensor(v, data, row_off, rules=None, compact=False, copy=True):
    """repetition_rows for a batch in tensors on the handle's GPU (wp_repetition_rows_device): data uint8, row_off int64 —
    a joined text and its doc_off, the compact form of quality_rows_tensor.  -> a dict of tensors on that device:
    "signals" (torch.int64 [14, n_rows]), "reasons" (the uint32 bitmasks as torch.int32), with compact "kept", "data" and
    "row_off" (what dedup_rows_tensor takes).  copy=False: views of the library's buffers, valid until the next call on
    this handle."""
    batches = W._ragged_tensors("repetition", v._device, [(data, row_off)], ids=False, offsets="offsets", s="")
    lib()
    return v._rows_device("repetition", _spec(rules, compact), batches, dict(compact=compact), copy, n_signals=len(REPETITION_SIGNALS))


def repetition_docs(v, docs, rules=None):
    """The documents of a list (str / bytes) that fail none of `rules` -> ([those documents as given], np.uint32 reasons
    of every document of docs); through repetition_rows over the documents back to back (no byte is added)."""
    docs = list(docs)
    bs = [W._bytes(d) for d in docs]
    r = repetition_rows(v, b"".join(bs), W._offsets_of([len(b) for b in bs]), rules=rules)
    return [d for d, x in zip(docs, r["reasons"]) if x == 0], r["reasons"]
