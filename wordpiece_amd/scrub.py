"""The scrub (include/wordpiece_amd_scrub.h): e-mail addresses and IPv4 addresses of every document replaced by
placeholders on the device, exactly — the PII step between the filters and the tokeniser of a corpus pipeline.  A submodule
beside the line filter: its functions take the Vocab handle first and go through the wrapper's shared intake and result
tables, where this module registers its layer.  The same address gets the same placeholder in every call (a fixed hash).

    from wordpiece_amd import scrub
    r = scrub.scrub_rows_tensor(v, f["data"], f["row_off"], compact=True)
    v.dedup_rows_tensor(r["data"], r["row_off"])
"""
import ctypes as C

import numpy as np

import wordpiece_amd as W

WP_SCRUB_EMAIL, WP_SCRUB_IPV4, WP_SCRUB_IP_KEEP_PRIVATE = 1, 2, 4
WP_SCRUB_WANT_MATCHES, WP_SCRUB_WANT_TEXT, WP_SCRUB_WANT_COMPACT = 1, 2, 4
# the signals (rows of "signals"), the document rules (bit k of reasons), the kinds of a match ("match_kind")
SCRUB_SIGNALS = ("bytes", "out_bytes", "at_signs", "emails", "email_bytes", "ips", "ip_bytes", "ips_left")
SCRUB_RULES = ("max_emails", "max_ips")
SCRUB_KINDS = ("email", "ipv4", "ipv4_left")
ABI_SYMBOLS = ["wp_scrub_rows", "wp_scrub_rows_device", "wp_get_scrub_stats"]
_PRESETS = {
    "default": dict(email=("email@example.com", "firstname.lastname@example.org"), ip=("192.0.2.1", "198.51.100.1", "203.0.113.1")),  # (RFC 2606, RFC 5737)
}


def scrub_replacements(name):
    """The placeholders of a named set as keyword arguments of the scrub calls: "default" -> {"email", "ip"}, two
    addresses in the reserved example domains and the three RFC 5737 documentation addresses."""
    if name not in _PRESETS:
        raise W.WordPieceError("scrub: no such replacements: %r (known: %s)" % (name, ", ".join(sorted(_PRESETS))))
    return {k: list(x) for k, x in _PRESETS[name].items()}


class ScrubSpec(C.Structure):
    """wp_scrub_spec: the arguments of a scrub call."""
    _fields_ = [("elem_bytes", C.c_int32), ("want", C.c_int32), ("kinds", C.c_int32), ("pad", C.c_int32), ("doc_limit", C.c_int64 * 2), ("n_email_repl", C.c_int32),
                ("n_ip_repl", C.c_int32), ("repl_pool", C.c_void_p), ("repl_off", C.c_void_p), ("reserved", C.c_int64)]


class ScrubResult(C.Structure):
    """wp_scrub_result: the arrays of a scrub call (host blocks, or device memory owned by the handle)."""
    _fields_ = [("signals", C.c_void_p), ("match_start", C.c_void_p), ("out_off", C.c_void_p), ("row_off", C.c_void_p), ("reasons", C.c_void_p),
                ("match_row", C.c_void_p), ("match_len", C.c_void_p), ("match_kind", C.c_void_p), ("match_repl", C.c_void_p), ("kept", C.c_void_p),
                ("out_data", C.c_void_p), ("data", C.c_void_p), ("n_rows", C.c_int64), ("n_matches", C.c_int64), ("n_out_elems", C.c_int64), ("n_kept", C.c_int64),
                ("n_elems", C.c_int64)]


class ScrubStats(C.Structure):
    """wp_scrub_stats: the statistics of the last scrub call (scrub_stats(v))."""
    _fields_ = [("n_rows", C.c_int64), ("n_bytes", C.c_int64), ("n_out_bytes", C.c_int64), ("n_matches", C.c_int64 * 3), ("rule_failed", C.c_int64 * 2),
                ("n_kept", C.c_int64)]


# the layer in the wrapper's tables (wordpiece_amd: _CORPUS_LAYERS, _RESULTS)
W._CORPUS_LAYERS["scrub"] = ("wp_scrub_rows", ScrubSpec, ScrubResult, ScrubStats, W._BATCH, W._BATCH)
W._RESULTS["scrub"] = (("signals", "i64", ("n_signals", "rows"), None), ("reasons", "u32", ("rows",), None), ("match_row", "i32", ("n_matches",), "matches"),
                       ("match_start", "i64", ("n_matches",), "matches"), ("match_len", "i32", ("n_matches",), "matches"),
                       ("match_kind", "i32", ("n_matches",), "matches"), ("match_repl", "i32", ("n_matches",), "matches"),
                       ("out_data", "elem", ("n_out_elems",), "text"), ("out_off", "off", ("rows",), "text"), ("kept", "i32", ("n_kept",), "compact"),
                       ("data", "elem", ("n_elems",), "compact"), ("row_off", "off", ("n_kept",), "compact"))


def lib():
    """The package's library with this layer's entry points bound; a library without them is an error."""
    L = W.lib()
    missing = [s for s in ABI_SYMBOLS if not hasattr(L, s)]
    if missing:
        raise W.WordPieceError("the library has no scrub: %s missing" % ", ".join(missing))
    if L.wp_scrub_rows.argtypes is None:
        vp, args = C.c_void_p, [C.POINTER(ScrubSpec), C.POINTER(ScrubResult)]
        L.wp_scrub_rows.argtypes = [vp] + W._BATCH + args
        L.wp_scrub_rows_device.argtypes = [vp] + W._BATCH + args
        L.wp_get_scrub_stats.argtypes = [vp, C.POINTER(ScrubStats)]
    return L


def _spec(kinds, keep_private, email, ip, rules, matches, text, compact):
    """-> (ScrubSpec, the arrays its pointers name: keep them until the call is over)"""
    bits = 0
    for kind in kinds:
        if kind not in SCRUB_KINDS[:2]:
            raise W.WordPieceError("scrub: no such kind: %r" % (kind,))
        bits |= 1 << SCRUB_KINDS.index(kind)
    default = _PRESETS["default"]
    email, ip = [W._bytes(x) for x in (default["email"] if email is None else email)], [W._bytes(x) for x in (default["ip"] if ip is None else ip)]
    limit = [-1] * 2
    for name, value in dict(rules or {}).items():
        if name not in SCRUB_RULES:
            raise W.WordPieceError("scrub: no such rule: %r" % (name,))
        limit[SCRUB_RULES.index(name)] = int(value)
    pool = np.frombuffer(b"".join(email + ip) + b"\0", dtype=np.uint8)
    off = W._offsets_of([len(b) for b in email + ip])
    want = (WP_SCRUB_WANT_MATCHES if matches else 0) | (WP_SCRUB_WANT_TEXT if text else 0) | (WP_SCRUB_WANT_COMPACT if compact else 0)
    spec = ScrubSpec(1, want, bits | (WP_SCRUB_IP_KEEP_PRIVATE if keep_private else 0), 0, (C.c_int64 * 2)(*limit), len(email), len(ip), pool.ctypes.data,
                     off.ctypes.data, 0)
    return spec, (pool, off)


def scrub_stats(v):
    """wp_scrub_stats of the last scrub call on v as a dict (n_rows -1: no such call yet)."""
    lib()
    return v._stats(ScrubStats, "wp_get_scrub_stats")


def scrub_rows(v, data, row_off, kinds=("email", "ipv4"), keep_private=False, email=None, ip=None, rules=None, matches=False, text=False, compact=False, raw=False):
    """The e-mail and IPv4 addresses of every row of a ragged batch of text found and replaced (wp_scrub_rows).  data /
    row_off: the batch as filter_lines takes it.  kinds: what is searched, of SCRUB_KINDS[:2]; keep_private: addresses of
    the private, loopback, link-local and multicast ranges stay ("ips_left").  email / ip: 1 to 16 placeholders of 0 to 64
    bytes each (str or bytes; None: scrub_replacements("default")); a match gets the one its lower-cased bytes hash to.
    rules: {name of SCRUB_RULES: limit}.
    -> {"signals": np.int64 [8, n_rows] (rows of SCRUB_SIGNALS), "reasons": np.uint32 [n_rows] (bit k: SCRUB_RULES[k])};
    matches: "match_row", "match_start", "match_len", "match_kind" (index of SCRUB_KINDS), "match_repl" per match in text
    order; text: "out_data" and "out_off", every row scrubbed; compact: "kept", "data", "row_off", the rows with reasons 0
    after the scrub, back to back.  raw: the data comes back as np.uint8."""
    batch = W._ragged_batch("scrub", data, row_off)
    if batch[0].dtype != np.uint8:
        raise W.WordPieceError("scrub: data must be text")
    lib()
    spec, hold = _spec(kinds, keep_private, email, ip, rules, matches, text, compact)
    res = v._rows_host("scrub", spec, [batch], dict(matches=matches, text=text, compact=compact), True, n_signals=len(SCRUB_SIGNALS))
    if not raw:
        res.update((k, res[k].tobytes()) for k in ("data", "out_data") if k in res)
    return res


def scrub_rows_tensor(v, data, row_off, kinds=("email", "ipv4"), keep_private=False, email=None, ip=None, rules=None, matches=False, text=False, compact=False,
                      copy=True):
    """scrub_rows for a batch in tensors on the handle's GPU (wp_scrub_rows_device): data uint8, row_off int64 — the
    compact form of filter_lines_tensor.  -> a dict of tensors on that device, the uint32 bitmask as torch.int32; with
    compact "kept", "data" and "row_off" (what dedup_rows_tensor and encode_rows_tensor take).  copy=False: views of the
    library's buffers, valid until the next call on this handle."""
    batches = W._ragged_tensors("scrub", v._device, [(data, row_off)], ids=False, offsets="offsets", s="")
    lib()
    spec, hold = _spec(kinds, keep_private, email, ip, rules, matches, text, compact)
    return v._rows_device("scrub", spec, batches, dict(matches=matches, text=text, compact=compact), copy, n_signals=len(SCRUB_SIGNALS))


def scrub_docs(v, docs, **how):
    """The documents of a list (str / bytes) through scrub_rows (its keywords) -> ([the documents with reasons 0,
    scrubbed, as bytes], np.uint32 reasons of every document of docs)."""
    bs = [W._bytes(d) for d in docs]
    r = scrub_rows(v, b"".join(bs), W._offsets_of([len(b) for b in bs]), compact=True, **how)
    off = r["row_off"]
    return [r["data"][off[k]:off[k + 1]] for k in range(len(r["kept"]))], r["reasons"]
