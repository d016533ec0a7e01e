"""Rows seen in earlier batches (include/wordpiece_amd_seen.h): a set of 64-bit row keys that lives on the Vocab handle, in
device memory, across calls — the exact dedup of a corpus that comes in shards.  A submodule beside the scrub: its functions
take the Vocab handle first and go through the wrapper's shared intake and result tables, where this module registers its
layer.  Membership is by key (the round-0 key of dedup_rows at 64 bits); no byte is compared.

    from wordpiece_amd import seen
    for shard in shards:
        r = seen.seen_rows_tensor(v, shard["data"], shard["row_off"], compact=True)   # the rows no shard before had
        v.encode_rows_tensor(r["data"], r["row_off"])
    np.save("seen.npy", seen.seen_keys(v))                                           # ... and seen_add_keys loads it again
"""
import ctypes as C

import numpy as np

import wordpiece_amd as W

WP_SEEN_WANT_KEYS, WP_SEEN_WANT_COMPACT = 1, 2
WP_SEEN_QUERY_ONLY = 1
WP_SEEN_MIN_SLOTS = 1024
SEEN_STATES = ("new", "repeat_batch", "before")  # the values of "state"
ABI_SYMBOLS = ["wp_seen_rows", "wp_seen_rows_device", "wp_seen_keys", "wp_seen_keys_device", "wp_seen_export", "wp_seen_export_device", "wp_seen_reserve",
               "wp_seen_clear", "wp_get_seen_stats"]


class SeenSpec(C.Structure):
    """wp_seen_spec: the arguments of a seen call."""
    _fields_ = [("elem_bytes", C.c_int32), ("want", C.c_int32), ("flags", C.c_int32), ("pad", C.c_int32), ("reserved", C.c_int64)]


class SeenResult(C.Structure):
    """wp_seen_result: the arrays of a seen call (host blocks, or device memory owned by the handle)."""
    _fields_ = [("state", C.c_void_p), ("first", C.c_void_p), ("kept", C.c_void_p), ("keys", C.c_void_p), ("row_off", C.c_void_p), ("data", C.c_void_p),
                ("n_rows", C.c_int64), ("n_kept", C.c_int64), ("n_elems", C.c_int64)]


class SeenStats(C.Structure):
    """wp_seen_stats: the last seen call and the set (seen_stats(v))."""
    _fields_ = [("n_rows", C.c_int64), ("n_new", C.c_int64), ("n_repeat_batch", C.c_int64), ("n_seen_before", C.c_int64), ("n_keys", C.c_int64),
                ("capacity", C.c_int64), ("n_grown", C.c_int64), ("n_probes", C.c_int64)]


# the layer in the wrapper's tables (wordpiece_amd: _CORPUS_LAYERS, _RESULTS, _KINDS); uint64 keys travel to torch as int64 bit patterns
W._KINDS["u64"] = (np.uint64, "<i8", "int64")
W._CORPUS_LAYERS["seen"] = ("wp_seen_rows", SeenSpec, SeenResult, SeenStats, W._BATCH, W._BATCH)
W._RESULTS["seen"] = (("state", "i32", ("rows",), None), ("first", "i32", ("rows",), None), ("keys", "u64", ("rows",), "keys"),
                      ("kept", "i32", ("n_kept",), "compact"), ("data", "elem", ("n_elems",), "compact"), ("row_off", "off", ("n_kept",), "compact"))


def lib():
    """The package's library with this layer's entry points bound; a library without them is an error."""
    L = W.lib()
    missing = [s for s in ABI_SYMBOLS if not hasattr(L, s)]
    if missing:
        raise W.WordPieceError("the library has no seen rows: %s missing" % ", ".join(missing))
    if L.wp_seen_keys.argtypes is None:
        vp, args = C.c_void_p, [C.POINTER(SeenSpec), C.POINTER(SeenResult)]
        L.wp_seen_rows.argtypes = [vp] + W._BATCH + args
        L.wp_seen_rows_device.argtypes = [vp] + W._BATCH + args
        L.wp_seen_keys.argtypes = [vp, vp, C.c_size_t] + args
        L.wp_seen_keys_device.argtypes = [vp, vp, C.c_size_t] + args
        L.wp_seen_export.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.wp_seen_export_device.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.wp_seen_reserve.argtypes = [vp, C.c_size_t]
        L.wp_seen_clear.argtypes = [vp]
        L.wp_get_seen_stats.argtypes = [vp, C.POINTER(SeenStats)]
    return L


def _spec(elem_bytes, insert, keys=False, compact=False):
    want = (WP_SEEN_WANT_KEYS if keys else 0) | (WP_SEEN_WANT_COMPACT if compact else 0)
    return SeenSpec(elem_bytes, want, 0 if insert else WP_SEEN_QUERY_ONLY, 0, 0)


def seen_stats(v):
    """wp_seen_stats on v as a dict: n_rows, n_new, n_repeat_batch, n_seen_before of the last seen call (n_rows -1: none
    yet); n_keys, capacity, n_grown of the set; n_probes, a figure for the probe script and no part of the contract."""
    lib()
    return v._stats(SeenStats, "wp_get_seen_stats")


def seen_rows(v, data, row_off, insert=True, keys=False, compact=False, raw=False):
    """Every row of a ragged batch against the set of the handle, and (insert) the new ones into it (wp_seen_rows).  data /
    row_off: the batch as dedup_rows takes it, text or int32 ids (row_off None: the lines of a text).
    -> {"state": np.int32 [n_rows] (0 new, 1 a smaller row of the batch has the key, 2 in the set before the call),
    "first": np.int32 [n_rows] (the smallest row of the batch with the key)}; keys: "keys" np.uint64 [n_rows]; compact:
    "kept", "data", "row_off", the rows of state 0 back to back.  insert=False asks only: the set stays as it is.
    raw: text comes back as np.uint8."""
    batch = W._ragged_batch("seen", data, row_off)
    lib()
    return v._rows_host("seen", _spec(batch[0].dtype.itemsize, insert, keys, compact), [batch], dict(keys=keys, compact=compact), raw)


def seen_rows_tensor(v, data, row_off, insert=True, keys=False, compact=False, copy=True):
    """seen_rows for a batch in tensors on the handle's GPU (wp_seen_rows_device): data uint8 or int32, row_off int64.
    -> a dict of tensors on that device; the uint64 "keys" come as torch.int64 bit patterns (torch has no uint64
    arithmetic), as uint32 masks come as int32.  With compact "kept", "data" and "row_off" are what dedup_rows_tensor and
    encode_rows_tensor take.  copy=False: views of the library's buffers, valid until the next call on this handle."""
    batches = W._ragged_tensors("seen", v._device, [(data, row_off)])
    lib()
    return v._rows_device("seen", _spec(batches[0][0].element_size(), insert, keys, compact), batches, dict(keys=keys, compact=compact), copy)


def seen_docs(v, docs, **how):
    """The documents of a list (str / bytes) through seen_rows (its keywords) -> ([the new documents as bytes], np.int32
    states of every document of docs)."""
    bs = [W._bytes(d) for d in docs]
    r = seen_rows(v, b"".join(bs), W._offsets_of([len(b) for b in bs]), compact=True, **how)
    off = r["row_off"]
    return [r["data"][off[k]:off[k + 1]] for k in range(len(r["kept"]))], r["state"]


def seen_add_keys(v, keys, insert=True):
    """Given keys against the set, and (insert) the new ones into it (wp_seen_keys): what loads a saved set and merges the
    sets of other handles, ranks or processes.  keys: uint64 (0 is taken as 1).  -> {"state", "first"} as seen_rows."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    if keys.ndim != 1:
        raise W.WordPieceError("seen: keys must be a flat uint64 array")
    out = SeenResult()
    W._check(lib().wp_seen_keys(v._h, keys.ctypes.data if keys.size else None, keys.size, C.byref(_spec(0, insert)), C.byref(out)))
    return W._host_result("seen", out, rows=keys.size)


def seen_add_keys_tensor(v, keys, insert=True, copy=True):
    """seen_add_keys for keys in a torch.int64 tensor (the bit patterns of the uint64 keys) on the handle's GPU
    (wp_seen_keys_device) -> {"state", "first"} as tensors there."""
    import torch
    if keys.dtype != torch.int64:
        raise W.WordPieceError("seen_add_keys_tensor needs int64 keys (the bit patterns of the uint64 keys)")
    W._flat_device_tensors("seen_add_keys_tensor", v._device, keys)
    torch.cuda.current_stream(keys.device).synchronize()  # the library runs on its own HIP streams
    out = SeenResult()
    W._check(lib().wp_seen_keys_device(v._h, C.c_void_p(keys.data_ptr()) if keys.numel() else None, keys.numel(), C.byref(_spec(0, insert)), C.byref(out)))
    return W._layer_result("seen", out, W._DeviceViews(keys.device, copy), rows=keys.numel())


def seen_keys(v):
    """All keys of the set, ascending (wp_seen_export) -> np.uint64 [n_keys]: the same whatever order the keys came in."""
    n = C.c_size_t(0)
    out = np.empty(seen_stats(v)["n_keys"], dtype=np.uint64)
    W._check(lib().wp_seen_export(v._h, out.ctypes.data if out.size else None, out.size, C.byref(n)))
    return out[:n.value]


def seen_keys_tensor(v):
    """seen_keys into a torch.int64 tensor (bit patterns) on the handle's GPU (wp_seen_export_device); ascending as uint64."""
    import torch
    n = C.c_size_t(0)
    out = torch.empty(seen_stats(v)["n_keys"], dtype=torch.int64, device=torch.device("cuda", torch.cuda.current_device() if v._device is None else v._device))
    W._check(lib().wp_seen_export_device(v._h, C.c_void_p(out.data_ptr()) if out.numel() else None, out.numel(), C.byref(n)))
    return out[:n.value]


def seen_reserve(v, n_keys):
    """Room for n_keys keys in advance (wp_seen_reserve): no call grows the table while the keys of the set and the rows
    of the call together stay within n_keys."""
    W._check(lib().wp_seen_reserve(v._h, int(n_keys)))


def seen_clear(v):
    """Empties the set and frees its memory (wp_seen_clear)."""
    W._check(lib().wp_seen_clear(v._h))
