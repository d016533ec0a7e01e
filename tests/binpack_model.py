"""The Python statement of wp_pack_best_fit (include/wordpiece_amd_binpack.h): the procedure of the header written
literally — a dict of deques, one unit at a time.  The pieces and their units come from tests/pack_model.py.  The
yardstick of tests/test_binpack_abi.py (the planner) and tests/test_gpu_binpack.py (the library, exactly)."""
import bisect
from collections import deque

import numpy as np

import pack_model as PM


def place(u, L):
    """units of u[k] cells, k in document order -> (row, slot, col) of every unit and the number of rows opened"""
    u = np.asarray(u, dtype=np.int64)
    assert len(u) == 0 or (u.min() >= 1 and u.max() <= L)
    row, slot, col = (np.zeros(len(u), np.int64) for _ in range(3))
    queues, caps, units_in, n_out = {}, [], [], 0  # caps: the capacities with a row queued, ascending
    for k in np.argsort(-u, kind="stable"):  # sigma: u descending, ties by k ascending
        at = bisect.bisect_left(caps, u[k])  # the smallest r >= u whose queue is not empty
        if at < len(caps):
            r = caps[at]
            j = queues[r].popleft()
            if not queues[r]:
                del queues[r], caps[at]
        else:
            r, j, n_out = L, n_out, n_out + 1
            units_in.append(0)
        row[k], slot[k], col[k] = j, units_in[j], L - r
        units_in[j] += 1
        if r - u[k] > 0:
            if r - u[k] not in queues:
                queues[r - u[k]] = deque()
                bisect.insort(caps, r - u[k])
            queues[r - u[k]].append(j)
    return row, slot, col, n_out


def pack(ids, row_splits, max_len, bos_id=-1, eos_id=-1, pad_id=0, long_docs=PM.LONG_SPLIT, want=7):
    """-> dict: the five blocks as pack_model.pack returns them, n_out, stats (the first eight fields of wp_binpack_stats
    and n_row_ranges), and u / row / slot / col of every piece."""
    ids, splits, L = np.asarray(ids, dtype=np.int32), np.asarray(row_splits, dtype=np.int64), int(max_len)
    doc, first, n, stats = PM.pieces(splits, L, PM.NEXT_FIT, bos_id, eos_id, long_docs)
    has_bos, has_eos = int(bos_id >= 0), int(eos_id >= 0)
    u = n + has_bos + has_eos
    row, slot, col, n_out = place(u, L)
    out = dict(input_ids=np.full((n_out, L), pad_id, np.int32), lengths=np.bincount(row, weights=u, minlength=n_out).astype(np.int32),
               segment_ids=np.zeros((n_out, L), np.int32) if want & PM.WANT_SEGMENTS else None,
               position_ids=np.zeros((n_out, L), np.int32) if want & PM.WANT_POSITIONS else None,
               source=np.full((n_out, L), -1, np.int32) if want & PM.WANT_SOURCE else None, n_out=n_out, u=u, row=row, slot=slot, col=col)
    k = np.repeat(np.arange(len(u), dtype=np.int64), u)  # the piece of every cell
    off = np.arange(len(k), dtype=np.int64) - np.repeat(np.cumsum(u) - u, u)
    is_bos, is_eos = (off == 0) & bool(has_bos), (off == u[k] - 1) & bool(has_eos)
    src = np.where(is_bos | is_eos, -1, splits[doc[k]] + first[k] + off - has_bos)
    val = np.where(is_bos, bos_id, np.where(is_eos, eos_id, ids[np.maximum(src, 0)] if len(ids) else 0)).astype(np.int32)
    r, c = row[k], col[k] + off
    out["input_ids"][r, c] = val
    if want & PM.WANT_SEGMENTS:
        out["segment_ids"][r, c] = 1 + slot[k]
    if want & PM.WANT_POSITIONS:
        out["position_ids"][r, c] = off
    if want & PM.WANT_SOURCE:
        out["source"][r, c] = src
    ends = np.stack([np.bincount(row, minlength=n_out), out["lengths"]], axis=1)  # units and cells of every row
    stats.update(n_out=n_out, n_cells=int(u.sum()), n_segments=len(u),
                 n_row_ranges=int(n_out > 0) + int(np.sum(np.any(ends[1:] != ends[:-1], axis=1))))
    out["stats"] = stats
    return out


def expand(runs, n_units):
    """the (row, slot, col, unit) of every sigma-rank from a run table, and whether the runs tile the ranks in order"""
    row, slot, col, unit = (np.full(n_units, -1, np.int64) for _ in range(4))
    at = 0
    for r in runs:
        assert r["first_rank"] == at and r["n_rows"] >= 1 and r["per_row"] >= 1, (r, at)
        m = int(r["n_rows"]) * int(r["per_row"])
        j, t = np.divmod(np.arange(m, dtype=np.int64), int(r["per_row"]))
        row[at:at + m], slot[at:at + m], col[at:at + m], unit[at:at + m] = r["row0"] + j, r["slot0"] + t, r["col0"] + t * r["unit"], r["unit"]
        at += m
    assert at == n_units
    return row, slot, col, unit
