"""The contract of the near-duplicate row clustering (include/wordpiece_amd.h, section "near-duplicate rows") in
executable form: the shingle hash, the permutations, the signatures, the band keys, the buckets by dict, the edges to the
head of a bucket and the components by union-find.  Nothing here knows of tiles, sorts, atomics or rounds; numpy only
carries the 64-bit arithmetic."""
import functools
import math

import numpy as np

G = 0x9e3779b97f4a7c15
MASK64 = (1 << 64) - 1
EMPTY = 0xffffffff
WANT_INVERSE, WANT_COMPACT, WANT_SIGNATURES = 1, 2, 4


def mix(h):
    """mix64 (csrc/group.h): the 64-bit finaliser, on a Python int"""
    h &= MASK64
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & MASK64
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & MASK64
    h ^= h >> 33
    return h


def _mix_np(h):
    """the same on a uint64 array (numpy wraps mod 2^64)"""
    h = h ^ (h >> np.uint64(33))
    h = h * np.uint64(0xff51afd7ed558ccd)
    h = h ^ (h >> np.uint64(33))
    h = h * np.uint64(0xc4ceb9fe1a85ec53)
    return h ^ (h >> np.uint64(33))


def shingle_x32(shingle, seed=0):
    """the 32-bit value of one shingle given as its bytes"""
    b = bytes(shingle)
    h = mix(mix(seed ^ G) ^ (len(b) | (1 << 41)))
    full = len(b) // 8
    for q in range(full):
        h = (mix(h ^ int.from_bytes(b[8 * q:8 * q + 8], "little")) + G) & MASK64
    h = mix(h ^ int.from_bytes(b[8 * full:], "little"))
    return (h ^ (h >> 32)) & 0xffffffff


def perm_ab(j, seed=0):
    """(a_j, b_j) of permutation j"""
    return mix(seed + (2 * j + 1) * G), mix(seed + (2 * j + 2) * G)


@functools.lru_cache(maxsize=64)
def _perm_arrays(n_perm, seed):
    ab = [perm_ab(j, seed) for j in range(n_perm)]
    return np.array([p[0] for p in ab], dtype=np.uint64), np.array([p[1] for p in ab], dtype=np.uint64)


def perm(j, x32, seed=0):
    a, b = perm_ab(j, seed)
    return ((a * x32 + b) & MASK64) >> 32


def row_x32(row, elem_bytes, k, seed=0):
    """the values of the shingles of one row (its bytes) -> uint64 array, one entry per shingle, in order"""
    row = bytes(row)
    n = len(row) // elem_bytes
    if n == 0:
        return np.zeros(0, dtype=np.uint64)
    if n < k:
        return np.array([shingle_x32(row, seed)], dtype=np.uint64)
    B = k * elem_bytes
    win = np.lib.stride_tricks.sliding_window_view(np.frombuffer(row, dtype=np.uint8), B)[::elem_bytes]
    padded = np.zeros((win.shape[0], (B // 8 + 1) * 8), dtype=np.uint8)
    padded[:, :B] = win
    words = padded.view("<u8")
    with np.errstate(over="ignore"):
        h = np.full(win.shape[0], mix(mix(seed ^ G) ^ (B | (1 << 41))), dtype=np.uint64)
        for q in range(B // 8):
            h = _mix_np(h ^ words[:, q]) + np.uint64(G)
        h = _mix_np(h ^ words[:, B // 8])  # (the rest zero-extended; a zero word where B is a multiple of 8)
    return (h ^ (h >> np.uint64(32))) & np.uint64(0xffffffff)


def signature(row, elem_bytes, k, n_perm, seed=0):
    """sig[j] = the minimum of P_j over the row's shingles -> uint32 [n_perm]; 0xffffffff without shingles"""
    x = row_x32(row, elem_bytes, k, seed)
    sig = np.full(n_perm, EMPTY, dtype=np.uint32)
    if x.size == 0:
        return sig
    a, b = _perm_arrays(n_perm, seed)
    step = max(1, (1 << 21) // x.size)  # (permutations per pass: the intermediate stays at a few MB)
    with np.errstate(over="ignore"):
        for j0 in range(0, n_perm, step):
            j1 = min(j0 + step, n_perm)
            sig[j0:j1] = ((a[j0:j1, None] * x[None, :] + b[j0:j1, None]) >> np.uint64(32)).min(axis=1).astype(np.uint32)
    return sig


def band_key(sig, band, r, seed=0):
    """the 64-bit key of one band of one signature"""
    h = mix(mix(seed ^ G) ^ (band + (1 << 42)))
    for t in range(r):
        h = (mix(h ^ int(sig[band * r + t])) + G) & MASK64
    return h


def lsh_min_agree(threshold, n_perm):
    return int(math.ceil(threshold * n_perm))


def rows_of(data, row_off, elem_bytes):
    data = bytes(data)
    off = [int(x) for x in row_off]
    n = len(off) - 1
    assert n >= 0 and (n == 0 or off[0] == 0) and all(off[i] <= off[i + 1] for i in range(n))
    assert n == 0 or off[n] * elem_bytes <= len(data)
    return [data[off[i] * elem_bytes:off[i + 1] * elem_bytes] for i in range(n)], off


def neardup_rows(data, row_off, elem_bytes=1, shingle=5, n_perm=128, bands=16, min_agree=0, seed=0, want=7):
    """-> {"cluster", "kept", "counts"} (lists), "inverse", "data" (bytes) + "row_off", "signatures" (uint32 [n_rows,
    n_perm]) on request, "edges" (the set of (member, head) pairs), and "stats": the statistics the contract fixes."""
    assert elem_bytes in (1, 4) and 1 <= shingle <= 64 and 1 <= n_perm <= 256 and bands >= 1 and n_perm % bands == 0
    assert 0 <= min_agree <= n_perm
    rows, off = rows_of(data, row_off, elem_bytes)
    n = len(rows)
    r = n_perm // bands
    cache = {}
    sigs = np.full((n, n_perm), EMPTY, dtype=np.uint32)
    for i, row in enumerate(rows):
        if row not in cache:
            cache[row] = signature(row, elem_bytes, shingle, n_perm, seed)
        sigs[i] = cache[row]
    # buckets: (row, band) pairs by key, in row-major order, so that the first member has the smallest row
    buckets = {}
    keys = {}
    for i, row in enumerate(rows):
        if not row:
            continue
        if row not in keys:
            keys[row] = [band_key(sigs[i], b, r, seed) for b in range(bands)]
        for b in range(bands):
            buckets.setdefault(keys[row][b], []).append(i)
    edges = set()
    n_buckets = n_candidates = n_edges = 0
    for members in buckets.values():
        if len(members) > 1:
            n_buckets += 1
        head = members[0]
        for m in members[1:]:
            if m == head:
                continue
            n_candidates += 1
            if min_agree == 0 or int((sigs[m] == sigs[head]).sum()) >= min_agree:
                n_edges += 1
                edges.add((m, head))
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for m, h in edges:
        a, b = find(m), find(h)
        if a != b:
            parent[max(a, b)] = min(a, b)
    cluster = [find(i) for i in range(n)]
    kept = [i for i in range(n) if cluster[i] == i]
    slot = {row: k for k, row in enumerate(kept)}
    counts = [0] * len(kept)
    for c in cluster:
        counts[slot[c]] += 1
    res = {"cluster": cluster, "kept": kept, "counts": counts, "edges": edges}
    if want & WANT_INVERSE:
        res["inverse"] = [slot[c] for c in cluster]
    if want & WANT_COMPACT:
        res["data"] = b"".join(rows[i] for i in kept)
        out = [0]
        for i in kept:
            out.append(out[-1] + len(rows[i]) // elem_bytes)
        res["row_off"] = out
    if want & WANT_SIGNATURES:
        res["signatures"] = sigs
    n_shingles = sum(0 if not row else max(len(row) // elem_bytes - shingle + 1, 1) for row in rows)
    res["stats"] = {"n_rows": n, "n_unique": len(kept), "n_empty": sum(1 for row in rows if not row), "n_elems": off[n] if n else 0,
                    "n_shingles": n_shingles, "n_buckets": n_buckets, "n_candidates": n_candidates, "n_edges": n_edges}
    return res


def join(rows, elem_bytes=1):
    """rows (bytes each, a multiple of elem_bytes) -> (data, row_off list)"""
    off = [0]
    for row in rows:
        assert len(row) % elem_bytes == 0
        off.append(off[-1] + len(row) // elem_bytes)
    return b"".join(rows), off
