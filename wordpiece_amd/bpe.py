"""Byte-level BPE on the device (include/wordpiece_amd_bpe.h): the GPT-2 pre-tokenizer pattern, a vocabulary and a ranked merge
list -> ids and row_splits in the shape encode_rows_tensor gives, so pack_sequences_tensor and binpack.pack_best_fit_tensor
take them unchanged.  A submodule beside the classifier: its functions take the Vocab handle first and go through the
wrapper's shared intake and result tables, where this module registers its layer.  A handle holds up to four models, one
per slot.

    from wordpiece_amd import bpe
    bpe.bpe_load_files(v, "vocab.json", "merges.txt")                   # slot 0
    r = bpe.bpe_encode_rows_tensor(v, data, row_off)                    # {"ids", "row_splits"}
    batch = binpack.pack_best_fit_tensor(v, r["ids"], r["row_splits"], max_len=2048, eos_id=eos)

Out of scope: other patterns (cl100k / Llama-3), ignore_merges, special tokens inside text, dropout, add_prefix_space,
decoding, learning merges.  The contract is the header, tests/bpe_model.py its executable form.
"""
import ctypes as C
import json

import numpy as np

import wordpiece_amd as W

WP_BPE_SLOTS = 4
WP_BPE_PATTERN_GPT2 = 0
WP_BPE_WANT_OFFSETS, WP_BPE_WANT_PIECES = 1, 2
# the sizes of the kernels that a text can straddle (csrc/bpe.h): the byte tile of the class and start pass, the bytes of
# the longest piece one lane merges, and of the longest one wave merges in LDS (longer ones take a workgroup each)
TILE_BYTES, SHORT_BYTES, MEDIUM_BYTES = 1024, 16, 256
ABI_SYMBOLS = ["wp_bpe_load", "wp_bpe_clear", "wp_bpe_encode_rows", "wp_bpe_encode_rows_device", "wp_get_bpe_stats"]


class BpeModel(C.Structure):
    """wp_bpe_model: the host arrays and the sizes of a model."""
    _fields_ = [("byte_id", C.c_void_p), ("merges", C.c_void_p), ("n_merges", C.c_int64), ("n_ids", C.c_int64), ("pattern", C.c_int32), ("reserved", C.c_int32)]


class BpeSpec(C.Structure):
    """wp_bpe_spec: the arguments of an encode call."""
    _fields_ = [("slot", C.c_int32), ("want", C.c_int32), ("pad", C.c_int32), ("pad2", C.c_int32), ("reserved", C.c_int64)]


class BpeResult(C.Structure):
    """wp_bpe_result: the arrays of an encode call (host blocks, or device memory owned by the handle)."""
    _fields_ = [("ids", C.c_void_p), ("row_splits", C.c_void_p), ("begin", C.c_void_p), ("end", C.c_void_p), ("piece_splits", C.c_void_p), ("n_rows", C.c_int64),
                ("n_ids", C.c_int64), ("n_pieces", C.c_int64)]


class BpeStats(C.Structure):
    """wp_bpe_stats: the last encode call on a slot and the slot's model (bpe_stats(v, slot))."""
    _fields_ = [(k, C.c_int64) for k in ("n_rows", "n_pieces", "n_ids", "max_piece", "n_short", "n_medium", "n_long", "n_merges", "model_ids", "table_slots")]


# the layer in the wrapper's tables (wordpiece_amd: _CORPUS_LAYERS, _RESULTS)
W._CORPUS_LAYERS["bpe"] = ("wp_bpe_encode_rows", BpeSpec, BpeResult, BpeStats, W._BATCH, W._BATCH)
W._RESULTS["bpe"] = (("ids", "i32", ("n_ids",), None), ("row_splits", "off", ("rows",), None), ("begin", "i32", ("n_ids",), "offsets"),
                     ("end", "i32", ("n_ids",), "offsets"), ("piece_splits", "off", ("n_pieces",), "pieces"))


def lib():
    """The package's library with this layer's entry points bound; a library without them is an error."""
    L = W.lib()
    missing = [s for s in ABI_SYMBOLS if not hasattr(L, s)]
    if missing:
        raise W.WordPieceError("the library has no byte-level BPE: %s missing" % ", ".join(missing))
    vp, args = C.c_void_p, [C.POINTER(BpeSpec), C.POINTER(BpeResult)]
    L.wp_bpe_load.argtypes = [vp, C.c_int, C.POINTER(BpeModel)]
    L.wp_bpe_clear.argtypes = [vp, C.c_int]
    L.wp_bpe_encode_rows.argtypes = [vp] + W._BATCH + args
    L.wp_bpe_encode_rows_device.argtypes = [vp] + W._BATCH + args
    L.wp_get_bpe_stats.argtypes = [vp, C.c_int, C.POINTER(BpeStats)]  # (the slot stands between the handle and the struct)
    return L


def bytes_to_unicode():
    """GPT-2's byte-level alphabet: {byte: the character that stands for it in vocab.json and merges.txt}.  The printable
    bytes stand for themselves, the others for U+0100 onwards in ascending order."""
    keep = list(range(0x21, 0x7F)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    rest = [b for b in range(256) if b not in keep]
    return {**{b: chr(b) for b in keep}, **{b: chr(256 + k) for k, b in enumerate(rest)}}


def bpe_load(v, vocab, merges, slot=0):
    """A model into slot 0..3 of the handle (wp_bpe_load), replacing the one there.  vocab: {token: id} in the byte-level
    alphabet, as vocab.json holds; merges: pairs (a, b) or lines "a b" in rank order, as merges.txt holds behind its
    "#version" line.  Translated here to byte_id int32 [256] and id triples (left, right, result); a byte or a merge whose
    tokens the vocabulary lacks is an error that names it."""
    alphabet = bytes_to_unicode()
    lacking = [b for b in range(256) if alphabet[b] not in vocab]
    if lacking:
        raise W.WordPieceError("bpe: the vocabulary lacks byte 0x%02x (%r)" % (lacking[0], alphabet[lacking[0]]))
    byte_id = np.array([vocab[alphabet[b]] for b in range(256)], dtype=np.int32)
    pairs = [tuple(m.split(" ")) if isinstance(m, str) else tuple(m) for m in merges]
    triples = np.zeros((len(pairs), 3), dtype=np.int32)
    for k, p in enumerate(pairs):
        if len(p) != 2:
            raise W.WordPieceError("bpe: merge %d is not a pair: %r" % (k, p))
        for tok in (p[0], p[1], p[0] + p[1]):
            if tok not in vocab:
                raise W.WordPieceError("bpe: merge %d (%r %r) needs %r, which the vocabulary lacks" % (k, p[0], p[1], tok))
        triples[k] = vocab[p[0]], vocab[p[1]], vocab[p[0] + p[1]]
    m = BpeModel(byte_id.ctypes.data, triples.ctypes.data if len(pairs) else None, len(pairs), max(vocab.values()) + 1, WP_BPE_PATTERN_GPT2, 0)
    W._check(lib().wp_bpe_load(v._h, int(slot), C.byref(m)))


def bpe_load_files(v, vocab_json, merges_txt, slot=0):
    """bpe_load from the two files of a GPT-2 style tokenizer: vocab.json and merges.txt (a first line "#version ..." and
    empty lines are passed over)."""
    with open(vocab_json, encoding="utf-8") as f:
        vocab = json.load(f)
    with open(merges_txt, encoding="utf-8") as f:
        lines = [ln.rstrip("\n") for ln in f]
    bpe_load(v, vocab, [ln for k, ln in enumerate(lines) if ln and not (k == 0 and ln.startswith("#version"))], slot)


def bpe_clear(v, slot=0):
    """Frees the model of the slot (wp_bpe_clear); the statistics of the slot start again."""
    W._check(lib().wp_bpe_clear(v._h, int(slot)))


def bpe_stats(v, slot=0):
    """wp_bpe_stats of the slot as a dict: n_rows, n_pieces, n_ids, max_piece, n_short, n_medium, n_long of the last call on
    it (n_rows -1: none yet); n_merges, model_ids, table_slots of its model (zeros: none loaded)."""
    s = BpeStats()
    W._check(lib().wp_get_bpe_stats(v._h, int(slot), C.byref(s)))
    return {k: getattr(s, k) for k, _ in s._fields_}


def _spec(slot, offsets, pieces):
    return BpeSpec(int(slot), (WP_BPE_WANT_OFFSETS if offsets else 0) | (WP_BPE_WANT_PIECES if pieces else 0), 0, 0, 0)


def bpe_encode_rows(v, data, row_off, slot=0, offsets=False, pieces=False):
    """Every document of a ragged batch of text encoded by the model of the slot (wp_bpe_encode_rows).  data / row_off: the
    batch as scrub_rows takes it (row_off None: the lines of a text).
    -> {"ids": np.int32 [n_ids], "row_splits": np.int64 [n_rows + 1]}; offsets: "begin" and "end" np.int32 [n_ids], the bytes
    of every id as offsets into its document; pieces: "piece_splits" np.int64 [n_pieces + 1], the first id of every piece."""
    batch = W._ragged_batch("bpe", data, row_off)
    if batch[0].dtype != np.uint8:
        raise W.WordPieceError("bpe: data must be text (bytes, uint8)")
    lib()
    return v._rows_host("bpe", _spec(slot, offsets, pieces), [batch], dict(offsets=offsets, pieces=pieces), True)


def bpe_encode_rows_tensor(v, data, row_off, slot=0, offsets=False, pieces=False, copy=True):
    """bpe_encode_rows for a batch in tensors on the handle's GPU (wp_bpe_encode_rows_device): data uint8, row_off int64.
    -> a dict of tensors on that device; "ids" and "row_splits" are what pack_sequences_tensor and
    binpack.pack_best_fit_tensor take.  copy=False: views of the library's buffers, valid until the next call on this handle."""
    batches = W._ragged_tensors("bpe", v._device, [(data, row_off)], ids=False)
    lib()
    return v._rows_device("bpe", _spec(slot, offsets, pieces), batches, dict(offsets=offsets, pieces=pieces), copy)


def bpe_encode_docs(v, docs, **how):
    """The documents of a list (str / bytes) through bpe_encode_rows (its keywords) -> its dict."""
    bs = [W._bytes(d) for d in docs]
    return bpe_encode_rows(v, b"".join(bs), W._offsets_of([len(b) for b in bs]), **how)
