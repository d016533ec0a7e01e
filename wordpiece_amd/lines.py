"""The line filter (include/wordpiece_amd_lines.h): single lines of a document dropped by rule, by phrase and by
repetition, and the documents handed back without them, on the device and exactly — the line-level step of C4 with CCNet's
duplicate-line removal.  A submodule beside the quality calls of the package: its functions take the Vocab handle first and
go through the wrapper's shared intake and result tables, where this module registers its layer.

    from wordpiece_amd import lines
    r = lines.filter_lines_tensor(v, q["data"], q["row_off"], rules="c4", compact=True)
    v.dedup_rows_tensor(r["data"], r["row_off"])
"""
import ctypes as C

import numpy as np

import wordpiece_amd as W

WP_LF_WANT_LINES, WP_LF_WANT_CUT, WP_LF_WANT_COMPACT = 1, 2, 4
WP_LF_PHRASE_BOUNDED, WP_LF_PHRASE_DOC = 1, 2
# the rules of a line (bit k of line_reasons; the first four take a limit), those of a document (bit k of reasons), the signals
LINE_RULES = ("min_words", "min_chars", "not_terminal", "ellipsis_end", "phrase", "duplicate")
DOC_RULES = ("min_kept_lines", "min_kept_words", "max_dropped_x1000", "max_doc_phrase_hits")
LINES_SIGNALS = ("bytes", "kept_bytes", "lines", "kept_lines", "line_chars", "kept_chars", "words", "kept_words", "failed_0", "failed_1", "failed_2",
                 "failed_3", "failed_4", "failed_5", "doc_phrase_hits")
ABI_SYMBOLS = ["wp_filter_lines", "wp_filter_lines_device", "wp_get_lines_stats"]
_PRESETS = {
    "c4": dict(rules={"min_words": 3, "not_terminal": 0, "min_kept_lines": 5, "max_doc_phrase_hits": 0},
               phrases=("javascript", "privacy policy", "terms of use", "cookie policy", "uses cookies", "use of cookies", "use cookies"),
               doc_phrases=("lorem ipsum", "{")),
}


def lines_rules(name):
    """The line filter of a published pipeline as keyword arguments of the filter calls: "c4" -> {"rules", "phrases",
    "doc_phrases"}.  It is the rule set as the T5 paper states it: a line stays where it has at least 3 words and ends in
    terminal punctuation; a line with "javascript" or one of the policy phrases goes; a document with "lorem ipsum" or
    "{" goes; min_kept_lines 5 stands in for the paper's five sentences.  All over THIS library's words and lines: parity
    with the TFDS implementation is not claimed, and these numbers could not be checked against it offline."""
    if name not in _PRESETS:
        raise W.WordPieceError("lines: no such preset: %r (known: %s)" % (name, ", ".join(sorted(_PRESETS))))
    p = _PRESETS[name]
    return dict(rules=dict(p["rules"]), phrases=list(p["phrases"]), doc_phrases=list(p["doc_phrases"]))


class LinesSpec(C.Structure):
    """wp_lines_spec: the arguments of a line-filter call."""
    _fields_ = [("elem_bytes", C.c_int32), ("want", C.c_int32), ("line_limit", C.c_int64 * 4), ("doc_limit", C.c_int64 * 4), ("dup_scope", C.c_int32),
                ("dup_min_chars", C.c_int32), ("n_phrases", C.c_int32), ("pad", C.c_int32), ("phrase_pool", C.c_void_p), ("phrase_off", C.c_void_p),
                ("phrase_flags", C.c_void_p), ("reserved", C.c_int64)]


class LinesResult(C.Structure):
    """wp_lines_result: the arrays of a line-filter call (host blocks, or device memory owned by the handle)."""
    _fields_ = [("signals", C.c_void_p), ("line_start", C.c_void_p), ("cut_off", C.c_void_p), ("row_off", C.c_void_p), ("reasons", C.c_void_p),
                ("line_reasons", C.c_void_p), ("line_row", C.c_void_p), ("line_len", C.c_void_p), ("kept", C.c_void_p), ("cut_data", C.c_void_p),
                ("data", C.c_void_p), ("n_rows", C.c_int64), ("n_lines", C.c_int64), ("n_cut_elems", C.c_int64), ("n_kept", C.c_int64), ("n_elems", C.c_int64)]


class LinesStats(C.Structure):
    """wp_lines_stats: the statistics of the last line-filter call (lines_stats(v))."""
    _fields_ = [("n_rows", C.c_int64), ("n_bytes", C.c_int64), ("n_lines", C.c_int64), ("n_kept_lines", C.c_int64), ("n_kept_bytes", C.c_int64),
                ("n_kept", C.c_int64), ("line_failed", C.c_int64 * 6), ("rule_failed", C.c_int64 * 4), ("n_phrase_matches", C.c_int64)]


# the layer in the wrapper's tables (wordpiece_amd: _CORPUS_LAYERS, _RESULTS)
W._CORPUS_LAYERS["lines"] = ("wp_filter_lines", LinesSpec, LinesResult, LinesStats, W._BATCH, W._BATCH)
W._RESULTS["lines"] = (("signals", "i64", ("n_signals", "rows"), None), ("reasons", "u32", ("rows",), None), ("line_row", "i32", ("n_lines",), "lines"),
                       ("line_start", "i64", ("n_lines",), "lines"), ("line_len", "i32", ("n_lines",), "lines"), ("line_reasons", "u32", ("n_lines",), "lines"),
                       ("cut_data", "elem", ("n_cut_elems",), "cut"), ("cut_off", "off", ("rows",), "cut"), ("kept", "i32", ("n_kept",), "compact"),
                       ("data", "elem", ("n_elems",), "compact"), ("row_off", "off", ("n_kept",), "compact"))


def lib():
    """The package's library with this layer's entry points bound; a library without them is an error."""
    L = W.lib()
    missing = [s for s in ABI_SYMBOLS if not hasattr(L, s)]
    if missing:
        raise W.WordPieceError("the library has no line filter: %s missing" % ", ".join(missing))
    if L.wp_filter_lines.argtypes is None:
        vp, args = C.c_void_p, [C.POINTER(LinesSpec), C.POINTER(LinesResult)]
        L.wp_filter_lines.argtypes = [vp] + W._BATCH + args
        L.wp_filter_lines_device.argtypes = [vp] + W._BATCH + args
        L.wp_get_lines_stats.argtypes = [vp, C.POINTER(LinesStats)]
    return L


def _spec(rules, phrases, doc_phrases, bounded, dup_scope, dup_min_chars, lines, cut, compact):
    """-> (LinesSpec, the arrays its pointers name: keep them until the call is over)"""
    if isinstance(rules, str):
        preset = lines_rules(rules)
        rules, phrases, doc_phrases = preset["rules"], list(preset["phrases"]) + list(phrases or ()), list(preset["doc_phrases"]) + list(doc_phrases or ())
    line_limit, doc_limit = [-1] * 4, [-1] * 4
    for name, value in dict(rules or {}).items():
        if name in LINE_RULES[:4]:
            line_limit[LINE_RULES.index(name)] = int(value)
        elif name in DOC_RULES:
            doc_limit[DOC_RULES.index(name)] = int(value)
        else:
            raise W.WordPieceError("lines: no such rule: %r" % (name,))
    bs = [W._bytes(p) for p in list(phrases or ()) + list(doc_phrases or ())]
    flags = [WP_LF_PHRASE_BOUNDED if bounded else 0] * len(phrases or ()) + [WP_LF_PHRASE_DOC | (WP_LF_PHRASE_BOUNDED if bounded else 0)] * len(doc_phrases or ())
    pool = np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8)
    off, flags = W._offsets_of([len(b) for b in bs]), np.asarray(flags, dtype=np.int32)
    want = (WP_LF_WANT_LINES if lines else 0) | (WP_LF_WANT_CUT if cut else 0) | (WP_LF_WANT_COMPACT if compact else 0)
    spec = LinesSpec(1, want, (C.c_int64 * 4)(*line_limit), (C.c_int64 * 4)(*doc_limit), int(dup_scope), int(dup_min_chars), len(bs), 0,
                     pool.ctypes.data if bs else None, off.ctypes.data if bs else None, flags.ctypes.data if bs else None, 0)
    return spec, (pool, off, flags)


def lines_stats(v):
    """wp_lines_stats of the last line-filter call on v as a dict (n_rows -1: no such call yet)."""
    lib()
    return v._stats(LinesStats, "wp_get_lines_stats")


def filter_lines(v, data, row_off, rules=None, phrases=(), doc_phrases=(), bounded=False, dup_scope=0, dup_min_chars=0, lines=False, cut=False, compact=False,
                 raw=False):
    """The lines of every row of a ragged batch of text judged, and the rows without the dropped ones (wp_filter_lines).
    data / row_off: the batch as quality_rows takes it.  rules: {name of LINE_RULES[:4] or DOC_RULES: limit}, or the name
    of a preset (lines_rules), whose phrases are then listed in front of the given ones.  phrases / doc_phrases: str or
    bytes, lower case, 1 to 32 bytes each: a line with a phrase is dropped, a doc phrase counts into "doc_phrase_hits";
    bounded: they match only between bytes that are no ASCII letter or digit and no byte >= 0x80.  dup_scope 1 / 2: a
    line of at least dup_min_chars characters that repeats an earlier line of its row / of the batch is dropped.
    -> {"signals": np.int64 [15, n_rows] (rows of LINES_SIGNALS), "reasons": np.uint32 [n_rows] (bit k: DOC_RULES[k])};
    lines: "line_row", "line_start", "line_len", "line_reasons" (bit k: LINE_RULES[k]) per line; cut: "cut_data" and
    "cut_off", every row without its dropped lines; compact: "kept", "data", "row_off", the rows with reasons 0 after the
    cut, back to back.  raw: the data comes back as np.uint8."""
    batch = W._ragged_batch("lines", data, row_off)
    if batch[0].dtype != np.uint8:
        raise W.WordPieceError("lines: data must be text")
    lib()
    spec, hold = _spec(rules, phrases, doc_phrases, bounded, dup_scope, dup_min_chars, lines, cut, compact)
    return v._rows_host("lines", spec, [batch], dict(lines=lines, cut=cut, compact=compact), raw, n_signals=len(LINES_SIGNALS))


def filter_lines_tensor(v, data, row_off, rules=None, phrases=(), doc_phrases=(), bounded=False, dup_scope=0, dup_min_chars=0, lines=False, cut=False,
                        compact=False, copy=True):
    """filter_lines for a batch in tensors on the handle's GPU (wp_filter_lines_device): data uint8, row_off int64 — a
    joined text and its doc_off, the compact form of quality_rows_tensor.  -> a dict of tensors on that device, the
    uint32 bitmasks as torch.int32; with compact "kept", "data" and "row_off" (what dedup_rows_tensor and
    encode_rows_tensor take).  copy=False: views of the library's buffers, valid until the next call on this handle."""
    batches = W._ragged_tensors("lines", v._device, [(data, row_off)], ids=False, offsets="offsets", s="")
    lib()
    spec, hold = _spec(rules, phrases, doc_phrases, bounded, dup_scope, dup_min_chars, lines, cut, compact)
    return v._rows_device("lines", spec, batches, dict(lines=lines, cut=cut, compact=compact), copy, n_signals=len(LINES_SIGNALS))


def filter_docs(v, docs, **how):
    """The documents of a list (str / bytes) through filter_lines (its keywords) -> ([the documents with reasons 0,
    without their dropped lines, as bytes], np.uint32 reasons of every document of docs)."""
    bs = [W._bytes(d) for d in docs]
    r = filter_lines(v, b"".join(bs), W._offsets_of([len(b) for b in bs]), compact=True, **how)
    off = r["row_off"]
    return [r["data"][off[k]:off[k + 1]] for k in range(len(r["kept"]))], r["reasons"]
