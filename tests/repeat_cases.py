"""The constructed inputs of the repeat tests.  The tile sizes are read from the kernels' headers: T, the window kernel's
tile (kOvlTile of csrc/overlap.h), and the element tile, the halo and the cut tile of csrc/repeat.h.  Every builder
returns (rows, elem_bytes, facts): the rows as bytes and what the construction promises — proven against the model on the
CPU in test_repeat_model.py before test_gpu_repeat.py relies on it."""
import os
import re

import numpy as np

from overlap_cases import distinct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _const(header, name):
    src = open(os.path.join(ROOT, "wordpiece_amd", "csrc", header)).read()
    return re.search(r"constexpr int %s = ([^;]+);" % name, src).group(1)


def tiles():
    """-> {"T": kOvlTile, "tile": kRepTile, "halo": kRepHalo, "cut": kRepCutTile}"""
    block = int(_const("common.h", "kBlock"))
    assert _const("repeat.h", "kRepHalo") == "kOvlMaxNgram" and _const("repeat.h", "kRepCutTile") == "kBlock * 4 * kRepCutWords"
    return {"T": int(_const("overlap.h", "kOvlTile")), "tile": int(_const("repeat.h", "kRepTile")), "halo": int(_const("overlap.h", "kOvlMaxNgram")),
            "cut": block * 4 * int(_const("repeat.h", "kRepCutWords"))}


def elems(values, eb):
    """elements of a small alphabet as a row: bytes, or ids"""
    a = np.asarray(values)
    assert a.size == 0 or eb == 4 or a.max() < 256
    return bytes(a.astype(np.uint8)) if eb == 1 else (a + 1000).astype(np.int32).tobytes()


def edge_starts(T, k):
    """(start, source) of the planted windows of edge_case: the repeat begins at 3T - k, 3T - 1 and 3T; its source lies in
    the tile of the start, in the one before and two tiles back (where that is in front of the start)"""
    out = []
    for start in (3 * T - k, 3 * T - 1, 3 * T):
        tile = start // T
        for src in (tile * T + 3, (tile - 1) * T + 5, (tile - 2) * T + 7, start - 1 if k > 1 else -1):
            if 0 <= src and src + k <= start:
                out.append((start, src))
    return out


def edge_case(T, k, eb, start, src, seed=1):
    """one row of 4T + 5 elements without a repeated window, but that the k elements at `src` are copied to `start`"""
    flat = distinct(4 * T + 5, eb, seed)
    flat[start:start + k] = flat[src:src + k]
    return [b"".join(flat)], eb, {"start": start, "src": src}


def row_end_case(T, k, eb, at, seed=2):
    """two rows, [0, at) and [at, at + T): the second begins with the last k + 2 elements of the first"""
    flat = distinct(at + T, eb, seed)
    flat[at:at + k + 2] = flat[at - k - 2:at]
    return [b"".join(flat[:at]), b"".join(flat[at:])], eb, {"repeats": [0, 3]}


def sized_case(n, k, eb, seed=3):
    """a batch of exactly n elements in rows of uneven lengths, a third of it copied from its first part"""
    flat = distinct(n, eb, seed)
    third = n // 3
    flat[2 * third:2 * third + third // 2] = flat[5:5 + third // 2]
    cuts = sorted({0, 1, third - 1, third + k, 2 * third + 9, n - 1, n})
    return [b"".join(flat[a:b]) for a, b in zip(cuts, cuts[1:])], eb, {"n": n}


def unit_rows_case(T, k, eb, seed=4):
    """T rows of exactly k elements, one window each; every odd row equals the even row in front of it"""
    flat = distinct(T * k, eb, seed)
    rows = [b"".join(flat[(i - i % 2) * k:(i - i % 2 + 1) * k]) for i in range(T)]
    return rows, eb, {"repeat_rows": list(range(1, T, 2))}


def periodic_case(n=3000, eb=1):
    """abab... of n elements"""
    return [elems(np.arange(n) % 2 + 97, eb)], eb, {}


def long_row_case(long_n=300_000, block_n=5_000, seed=5):
    """a row of 300,000 ids between 50 rows of 20: the block of its first 5,000 ids stands again at 50,000, 120,000 and
    250,000; the short rows behind it begin with 15 ids of the block"""
    ids = np.random.RandomState(seed).permutation(long_n + 2000).astype(np.int32)
    long_row, short = ids[:long_n].copy(), ids[long_n:]
    at = [50_000, 120_000, 250_000]
    for a in at:
        long_row[a:a + block_n] = long_row[:block_n]
    rows = [short[20 * i:20 * i + 20].tobytes() for i in range(25)] + [long_row.tobytes()]
    rows += [np.concatenate((long_row[100 * i:100 * i + 15], short[500 + 20 * i:505 + 20 * i])).tobytes() for i in range(25)]
    return rows, 4, {"long": 25, "at": at, "block": block_n}


def multiplicity_case(k, eb, seed=6):
    """windows that occur once, twice, three times and a thousand times"""
    rng = np.random.RandomState(seed)
    a, b, c = (elems(rng.randint(0, 100, k + 4), eb) for _ in range(3))
    fill = [elems(rng.randint(100, 120, 9), eb) for _ in range(6)]
    one = elems(np.zeros(1000 + k - 1, dtype=np.int64) + 125, eb)  # (1000 windows of one element repeated)
    rows = [fill[0] + a, fill[1] + b + fill[2] + c, one, fill[3] + b, c + fill[4], b"", fill[5] + c[:k * eb]]
    return rows, eb, {}


def cut_case(k, eb, cut_tile, seed=7):
    """covered spans at the start, in the middle and at the end of rows, rows that become empty, kept runs that begin at
    every output alignment, and a cut tile boundary inside a kept run and inside a covered run"""
    rng = np.random.RandomState(seed)
    tmpl = elems(rng.randint(0, 100, k + 6), eb)
    rows = [tmpl]
    for phase in range(4):  # (kept runs of 5 + phase elements between covered ones: every output alignment)
        body = [elems(rng.randint(100, 120, 5 + phase), eb) for _ in range(3)]
        rows += [tmpl + body[0], body[1] + tmpl + body[2], body[0][:3 * eb] + tmpl, tmpl, b""]
    pad = elems(rng.randint(100, 120, 1), eb)
    n = sum(len(r) for r in rows) // eb
    kept_run = b"".join(distinct(cut_tile - n + 200, eb, seed))  # the first cut tile boundary lies inside this kept run
    rows += [kept_run]
    n += len(kept_run) // eb
    covered_run = pad * ((2 * cut_tile - 40 - n) % cut_tile) + tmpl * 12  # ... and the second one inside this covered run
    rows += [covered_run, tmpl[:k * eb], pad * 3]
    rows += [elems(np.arange(j % 3 + 1) + 121 + 4 * j, eb) + tmpl for j in range(6)]  # (kept runs of 1, 2 and 3 elements)
    return rows, eb, {"empty": [4, 5]}


def utf8_pair():
    """the copyright sign and an e with acute in front of the same text: the bytes from the shared A9 on are equal"""
    text = "ab cd ef gh"
    return ["©" + text, "é" + text], text
