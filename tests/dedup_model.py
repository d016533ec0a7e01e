"""The contract of the duplicate-row removal (include/wordpiece_amd.h, section "duplicate rows") in executable form: a
plain dict from the bytes of a row to the index of its first occurrence.  Nothing here knows of chunks, hashes or rounds."""
import numpy as np


def dedup_rows(data, row_off, elem_bytes=1, want=3):
    """data: bytes (elem_bytes per element); row_off: n_rows + 1 ascending element offsets from 0; want: bit 1 inverse,
    bit 2 compact.  -> {"first", "kept", "counts"} (lists), "inverse" / "data" (bytes) and "row_off" on request, and
    "stats": the statistics that depend on no hash."""
    data = bytes(data)
    off = [int(x) for x in row_off]
    n = len(off) - 1
    assert n >= 0 and (n == 0 or off[0] == 0) and all(off[i] <= off[i + 1] for i in range(n))
    assert n == 0 or off[n] * elem_bytes <= len(data)
    seen = {}
    first, kept, counts = [], [], []
    for i in range(n):
        row = data[off[i] * elem_bytes:off[i + 1] * elem_bytes]
        k = seen.setdefault(row, len(kept))
        if k == len(kept):
            kept.append(i)
            counts.append(0)
        counts[k] += 1
        first.append(kept[k])
    res = {"first": first, "kept": kept, "counts": counts}
    if want & 1:
        slot = {r: k for k, r in enumerate(kept)}
        res["inverse"] = [slot[f] for f in first]
    if want & 2:
        rows = [data[off[i] * elem_bytes:off[i + 1] * elem_bytes] for i in kept]
        res["data"] = b"".join(rows)
        out = [0]
        for r in rows:
            out.append(out[-1] + len(r) // elem_bytes)
        res["row_off"] = out
    res["stats"] = {"n_rows": n, "n_unique": len(kept), "n_empty": sum(1 for i in range(n) if off[i] == off[i + 1]),
                    "n_elems": off[n] if n else 0}
    return res


def join(rows, elem_bytes=1):
    """rows (bytes each, a multiple of elem_bytes) -> (data, row_off list)"""
    off = [0]
    for r in rows:
        assert len(r) % elem_bytes == 0
        off.append(off[-1] + len(r) // elem_bytes)
    return b"".join(rows), off


def dedup_fixed(rows2d):
    """the same answer for fixed-length rows (a 2-D integer array), through numpy.unique: for batches too large for the dict"""
    _, idx, inv, cnt = np.unique(rows2d, axis=0, return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    order = np.argsort(idx, kind="stable")  # numpy sorts by value: back to the order of first occurrence
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    return {"first": idx[inv].astype(np.int32), "kept": idx[order].astype(np.int32), "counts": cnt[order].astype(np.int64),
            "inverse": rank[inv].astype(np.int32)}
