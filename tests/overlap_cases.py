"""The constructed inputs of the overlap tests.  T is the window kernel's tile (positions per workgroup, kOvlTile of
csrc/overlap.h).  Every builder returns (rows, refs, elem_bytes, facts): the corpus rows and the reference rows as bytes,
and what the construction promises — proven against the model on the CPU in test_overlap_model.py before
test_gpu_overlap.py relies on it."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tile():
    src = open(os.path.join(ROOT, "wordpiece_amd", "csrc", "overlap.h")).read()
    return int(re.search(r"constexpr int kOvlTile = (\d+);", src).group(1))


def distinct(n, elem_bytes, seed):
    """n elements as a list of element byte strings, no window of which repeats: ids are a permutation; text is a
    counter in base 200 whose digit groups open with a byte from another range, so that no window of 4 or more bytes
    repeats (shorter text windows may)."""
    rng = np.random.RandomState(seed)
    if elem_bytes == 4:
        ids = rng.permutation(n).astype(np.int32) + 1000
        return [ids[i:i + 1].tobytes() for i in range(n)]
    out = []
    i = 0
    while len(out) < n:
        out += [bytes([201 + i % 50]), bytes([i % 200]), bytes([i // 200 % 200]), bytes([i // 40000 % 200])]
        i += 1
    return out[:n]


def tile_edge_case(T, k, elem_bytes, seed=1):
    """one row of 3T + 5 elements; planted: the windows that begin at T - k .. T + 1 (the first ends exactly at T, the
    others cross into the halo) and the window at the very last position, each a reference row of its own, shuffled, with
    decoys between them"""
    flat = distinct(3 * T + 5, elem_bytes, seed)
    n = len(flat)
    planted = sorted(set(range(max(T - k, 0), T + 2)) | {n - k})
    if elem_bytes == 4:  # (ids the row does not hold; for text the counter goes on)
        decoys = [np.array([5_000_000 + i], dtype=np.int32).tobytes() for i in range(3 * k)]
    else:
        decoys = distinct(n + 8 + 3 * k, elem_bytes, seed)[n + 8:]
    refs = [b"".join(flat[p:p + k]) for p in planted] + [b"".join(decoys[:k]), b"".join(decoys[k:3 * k])]
    order = np.random.RandomState(seed).permutation(len(refs))
    return [b"".join(flat)], [refs[i] for i in order], elem_bytes, {"planted": planted, "n": n}


def boundary_case(T, k, elem_bytes, at, seed=2):
    """two rows, [0, at) and [at, at + T); the reference row is the k elements around the boundary, which no row holds"""
    assert k >= 2
    flat = distinct(at + T, elem_bytes, seed)
    s = at - k // 2
    return [b"".join(flat[:at]), b"".join(flat[at:])], [b"".join(flat[s:s + k])], elem_bytes, {"straddle": s, "flat": b"".join(flat)}


def unit_rows_case(T, k, elem_bytes, seed=3):
    """T rows of exactly k elements, one window each; every third one is a reference row"""
    flat = distinct(T * k, elem_bytes, seed)
    rows = [b"".join(flat[i * k:(i + 1) * k]) for i in range(T)]
    return rows, rows[::3], elem_bytes, {"hit_rows": list(range(0, T, 3))}


def long_row_case(k=13, long_n=300_000, seed=4):
    """a row of 300,000 ids between 50 rows of 20; of every 400 windows of the long row the first 100 are planted, as one
    reference row of 100 + k - 1 ids per burst: a quarter of its windows hit, and covered is a proper union"""
    ids = np.random.RandomState(seed).permutation(long_n + 1000).astype(np.int32)
    long_row, short = ids[:long_n], ids[long_n:]
    rows = [short[20 * i:20 * i + 20].tobytes() for i in range(25)] + [long_row.tobytes()] + [short[500 + 20 * i:520 + 20 * i].tobytes() for i in range(25)]
    bursts = list(range(0, long_n - 100 - k, 400))
    refs = [long_row[s:s + 100 + k - 1].tobytes() for s in bursts]
    return rows, refs, 4, {"long": 25, "bursts": bursts, "hits": 100 * len(bursts), "covered": (100 + k - 1) * len(bursts)}
