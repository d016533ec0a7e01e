"""Best-fit-decreasing packing (include/wordpiece_amd_binpack.h): long documents cut into chunks of at most one row, the
chunks packed longest first, each into the fullest row that still takes it — near-full rows, and only a document longer
than a row is ever cut (Ding et al., "Fewer Truncations Improve Language Modeling", ICML 2024).  A submodule beside the
pack calls of the package: its functions take the Vocab handle first and return what pack_sequences returns.

    from wordpiece_amd import binpack
    ids, splits = v.encode_rows_tensor(text, doc_off, copy=False)
    batch = binpack.pack_best_fit_tensor(v, ids, splits, max_len=512, eos_id=sep)
"""
import ctypes as C

import numpy as np

import wordpiece_amd as W

WP_BINPACK_MAX_LEN = 8192
ABI_SYMBOLS = ["wp_pack_best_fit", "wp_pack_best_fit_device", "wp_binpack_plan", "wp_get_binpack_stats"]
_I32, _I64 = C.c_int32, C.c_int64


class BinpackSpec(C.Structure):
    """wp_binpack_spec: the arguments of a best-fit pack call (bos_id / eos_id -1: none)."""
    _fields_ = [(k, _I32) for k in ("max_len", "bos_id", "eos_id", "pad_id", "long_docs", "want", "reserved0", "reserved1")]


class BinpackStats(C.Structure):
    """wp_binpack_stats: the statistics of the last best-fit pack call (binpack_stats(v))."""
    _fields_ = [(k, _I64) for k in ("n_docs", "n_empty", "n_cut", "n_ids_cut", "n_pieces", "n_out", "n_cells", "n_segments", "n_runs", "n_row_ranges")]


class BinpackRun(C.Structure):
    """wp_binpack_run: n_rows rows from row0 on take per_row units of `unit` cells each, from sigma-rank first_rank on."""
    _fields_ = [("first_rank", _I64), ("row0", _I64), ("n_rows", _I64), ("unit", _I32), ("per_row", _I32), ("slot0", _I32), ("col0", _I32)]


class BinpackRowRange(C.Structure):
    """wp_binpack_row_range: n_rows rows from row0 on that ended with the same number of units and of cells."""
    _fields_ = [("row0", _I64), ("n_rows", _I64), ("first_unit", _I64), ("first_cell", _I64), ("units_per_row", _I32), ("cells_per_row", _I32)]


class BinpackPlan(C.Structure):
    """wp_binpack_plan_result: the counts and the two tables of a plan (each freed with wp_free)."""
    _fields_ = [("n_out", _I64), ("n_units", _I64), ("n_cells", _I64), ("n_runs", _I64), ("n_row_ranges", _I64), ("runs", C.POINTER(BinpackRun)),
                ("row_ranges", C.POINTER(BinpackRowRange))]


def lib():
    """The package's library with this layer's entry points bound; a library without them is an error."""
    L = W.lib()
    missing = [s for s in ABI_SYMBOLS if not hasattr(L, s)]
    if missing:
        raise W.WordPieceError("the library has no best-fit packing: %s missing" % ", ".join(missing))
    if L.wp_pack_best_fit.argtypes is None:
        vp, sp, pp, np_ = C.c_void_p, C.POINTER(BinpackSpec), C.POINTER(W.Packed), C.POINTER(C.c_size_t)
        L.wp_pack_best_fit.argtypes = [vp, C.POINTER(_I32), C.POINTER(_I64), C.c_size_t, sp, pp, np_]
        L.wp_pack_best_fit_device.argtypes = [vp, vp, vp, C.c_size_t, sp, pp, C.c_size_t, np_]
        L.wp_binpack_plan.argtypes = [C.POINTER(_I64), _I32, C.POINTER(BinpackPlan)]
        L.wp_get_binpack_stats.argtypes = [vp, C.POINTER(BinpackStats)]
    return L


def _spec(max_len, bos_id, eos_id, pad_id, long_docs, want):
    p = W._pack_spec(max_len, "next_fit", bos_id, eos_id, pad_id, long_docs, want)  # (the names and the checks of the pack calls)
    return BinpackSpec(p.max_len, p.bos_id, p.eos_id, p.pad_id, p.long_docs, p.want, 0, 0)


def _table(ptr, n, struct):
    """a malloc'd table of the planner as a numpy structured array of its own; the block is freed"""
    if not n:
        return np.zeros(0, dtype=np.dtype(struct))
    out = np.ctypeslib.as_array(ptr, shape=(n,)).copy()
    W.lib().wp_free(ptr)
    return out


def plan_best_fit(hist_or_lengths, max_len, lengths=False):
    """The rows of a best-fit-decreasing packing from the unit lengths alone (wp_binpack_plan; no GPU needed).
    hist_or_lengths: hist[u], u in 0 .. max_len, the number of units of u cells — or, with lengths=True, the unit lengths
    themselves.  -> {"n_out", "n_units", "n_cells", "runs", "row_ranges"}: the tables as numpy structured arrays with
    the fields of BinpackRun and BinpackRowRange.  n_out is what pack_best_fit_tensor takes as n_out."""
    L = int(max_len)
    a = np.asarray(hist_or_lengths, dtype=np.int64)
    if a.ndim != 1:
        raise W.WordPieceError("binpack: the histogram (or the lengths) must be a 1-d array")
    if lengths:
        if len(a) and (a.min() < 1 or a.max() > L):
            raise W.WordPieceError("binpack: a unit has 1 to max_len cells")
        a = np.bincount(a, minlength=L + 1).astype(np.int64)
    if 1 <= L <= WP_BINPACK_MAX_LEN and len(a) != L + 1:
        raise W.WordPieceError("binpack: the histogram has max_len + 1 entries")
    a = np.ascontiguousarray(a)
    out = BinpackPlan()
    W._check(lib().wp_binpack_plan(a.ctypes.data_as(C.POINTER(_I64)), L, C.byref(out)))
    return dict(n_out=out.n_out, n_units=out.n_units, n_cells=out.n_cells, runs=_table(out.runs, out.n_runs, BinpackRun),
                row_ranges=_table(out.row_ranges, out.n_row_ranges, BinpackRowRange))


def binpack_stats(v):
    """wp_binpack_stats of the last best-fit pack call on v as a dict (n_docs -1: no such call yet)."""
    lib()
    return v._stats(BinpackStats, "wp_get_binpack_stats")


def pack_best_fit(v, ids, row_splits, max_len=128, bos_id=None, eos_id=None, pad_id=0, long_docs="split",
                  want=("segment_ids", "position_ids", "source")):
    """Several encoded documents per row, by best-fit decreasing (wp_pack_best_fit): ids int32 [n] with row_splits int64
    [n_docs + 1], as Vocab.pack_sequences takes them, and the same dict of numpy int32 arrays back.  long_docs "split"
    cuts a document longer than a row into chunks of a row, "truncate" keeps its first chunk; the chunks go into rows
    longest first.  source[r, c] is the index into ids of an id cell: the rows no longer follow document order."""
    a = np.ascontiguousarray(ids, dtype=np.int32)
    splits = np.ascontiguousarray(row_splits, dtype=np.int64)
    if a.ndim != 1 or splits.ndim != 1 or len(splits) < 1:
        raise W.WordPieceError("ids must be a 1-d array and row_splits a 1-d array of n_docs + 1 entries")
    if splits[-1] > len(a):
        raise W.WordPieceError("row_splits end behind the ids")
    spec = _spec(max_len, bos_id, eos_id, pad_id, long_docs, want)
    out, n = W.Packed(), C.c_size_t()
    W._check(lib().wp_pack_best_fit(v._h, W._i32_ptr(a), W._i64_ptr(splits), len(splits) - 1, C.byref(spec), C.byref(out), C.byref(n)))
    return W._packed_result(out, n.value, int(max_len), spec.want)


def pack_best_fit_tensor(v, ids, row_splits, max_len=128, bos_id=None, eos_id=None, pad_id=0, long_docs="split",
                         want=("segment_ids", "position_ids", "source"), n_out=None, out=None):
    """pack_best_fit for tensors on the handle's GPU (wp_pack_best_fit_device), with the semantics of
    Vocab.pack_sequences_tensor: int32 tensors written by the library, nothing but a histogram of at most max_len + 1
    counters leaves the device.  n_out: the row count if it is known (plan_best_fit gives it; an upper bound will do);
    without it the rows are sized by 2 (n + 2 n_docs) / max_len + 1 — two rows of a best-fit packing hold more than
    max_len cells between them — and the call runs twice where the chunks of split documents need more.  out: as there."""
    n_docs = W._pack_tensor_args(v, ids, row_splits)
    L = int(max_len)
    spec = _spec(L, bos_id, eos_id, pad_id, long_docs, want)
    if n_out is not None:
        cap = int(n_out)
    else:
        cap = 2 * (ids.numel() + 2 * n_docs) // L + 1
        if spec.long_docs == W.WP_PACK_LONG_TRUNCATE:
            cap = min(n_docs, cap)  # (a document gives a row at most)
    return W._pack_tensors(v, lib().wp_pack_best_fit_device, spec, ids, row_splits, L, cap, out)
