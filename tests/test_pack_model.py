"""The model of wp_pack_sequences (tests/pack_model.py) against independent formulations — a plain next-fit loop, a sliced
concatenation — its properties on seeded cases, the worked examples of the contract, and the tile / spine / apply
decomposition of csrc/packing.h run in Python with tiny tiles (no GPU, no library)."""
import random

import numpy as np
import pytest

import pack_model as M


def units_of(ids, splits, L, mode, bos, eos, long_docs):
    """the units as plain lists of (value, source) — written cell by cell, nothing shared with the model"""
    s = (bos >= 0) + (eos >= 0)
    B = L - s
    units = []
    for i in range(len(splits) - 1):
        lo, hi = splits[i], splits[i + 1]
        if lo == hi:
            continue
        if mode == M.STREAM:
            cuts = [(lo, hi)]
        elif long_docs == M.LONG_TRUNCATE:
            cuts = [(lo, min(hi, lo + B))]
        else:
            cuts = [(a, min(a + B, hi)) for a in range(lo, hi, B)]
        for a, b in cuts:
            units.append(([(bos, -1)] if bos >= 0 else []) + [(ids[x], x) for x in range(a, b)] + ([(eos, -1)] if eos >= 0 else []))
    return units


def plain_pack(ids, splits, L, mode, bos, eos, pad, long_docs):
    """rows of (value, segment, position, source) by the loops a reader would write first"""
    units = units_of(ids, splits, L, mode, bos, eos, long_docs)
    rows = []
    if mode == M.STREAM:
        flat = [(v, src, ui, j) for ui, u in enumerate(units) for j, (v, src) in enumerate(u)]
        for at in range(0, len(flat), L):
            row, seg, begin = [], 1, 0
            for c, (v, src, ui, j) in enumerate(flat[at:at + L]):
                if j == 0 and c > 0:
                    seg, begin = seg + 1, c
                elif j == 0:
                    begin = 0
                row.append((v, seg, c - begin, src))
            rows.append(row)
    else:
        row, seg = [], 0
        for u in units:
            assert len(u) <= L
            if row and len(row) + len(u) > L:  # next fit: a unit that does not fit opens a row
                rows.append(row)
                row, seg = [], 0
            seg += 1
            row += [(v, seg, j, src) for j, (v, src) in enumerate(u)]
        if row:
            rows.append(row)
    return rows


def assert_same(out, rows, L, pad):
    assert out["n_out"] == len(rows)
    for r, row in enumerate(rows):
        full = row + [(pad, 0, 0, -1)] * (L - len(row))
        assert out["lengths"][r] == len(row) and 1 <= len(row) <= L
        assert out["input_ids"][r].tolist() == [c[0] for c in full]
        assert out["segment_ids"][r].tolist() == [c[1] for c in full]
        assert out["position_ids"][r].tolist() == [c[2] for c in full]
        assert out["source"][r].tolist() == [c[3] for c in full]


def random_case(rng):
    L = rng.choice([1, 2, 3, 4, 5, 7, 8, 16, 33])
    bos = rng.choice([-1, 101])
    eos = rng.choice([-1, 102])
    while L - (bos >= 0) - (eos >= 0) < 1:
        L += 1
    n_docs = rng.randrange(0, 14)
    top = rng.choice([1, 3, L, 3 * L + 2])
    lens = [0 if rng.random() < 0.2 else rng.randrange(1, top + 1) for _ in range(n_docs)]
    splits = [0]
    for l in lens:
        splits.append(splits[-1] + l)
    ids = [1000 + x for x in range(splits[-1])]
    return ids, splits, L, bos, eos


@pytest.mark.parametrize("seed", range(6))
def test_model_against_plain_loops(seed):
    rng = random.Random(seed)
    for _ in range(500):  # 3,000 cases over the seeds, every mode each
        ids, splits, L, bos, eos = random_case(rng)
        for mode, long_docs in ((M.NEXT_FIT, M.LONG_TRUNCATE), (M.NEXT_FIT, M.LONG_SPLIT), (M.STREAM, M.LONG_TRUNCATE)):
            out = M.pack(ids, splits, L, mode, bos, eos, 7, long_docs)
            assert_same(out, plain_pack(ids, splits, L, mode, bos, eos, 7, long_docs), L, 7)
            # properties
            src = out["source"][out["source"] >= 0]
            assert np.all(np.diff(src) > 0)
            if not (mode == M.NEXT_FIT and long_docs == M.LONG_TRUNCATE):
                assert src.tolist() == list(range(len(ids)))
            cells = out["source"] >= 0
            assert np.array_equal(out["input_ids"][cells], np.asarray(ids, np.int32)[out["source"][cells]])
            N = sum(len(u) for u in units_of(ids, splits, L, mode, bos, eos, long_docs))
            st = out["stats"]
            assert int(out["lengths"].sum()) == N == st["n_cells"]
            assert st["n_segments"] == int(out["segment_ids"].max(axis=1).sum()) if out["n_out"] else st["n_segments"] == 0
            assert st["n_docs"] == len(splits) - 1 and st["n_empty"] == sum(a == b for a, b in zip(splits, splits[1:]))
            if mode == M.STREAM:
                assert out["n_out"] == (N + L - 1) // L


def test_stream_is_a_sliced_concatenation():
    rng = random.Random(99)
    for _ in range(300):
        ids, splits, L, bos, eos = random_case(rng)
        flat = [v for u in units_of(ids, splits, L, M.STREAM, bos, eos, 0) for v, _ in u]
        out = M.pack(ids, splits, L, M.STREAM, bos, eos, -5)
        rows = [flat[a:a + L] for a in range(0, len(flat), L)]
        assert out["input_ids"].tolist() == [r + [-5] * (L - len(r)) for r in rows]


@pytest.mark.parametrize("T", [4, 8, 16])
def test_rows_by_tiles(T):
    """the orbit of next through tiles of T pieces, L below and above T; with L > T the chain jumps over tiles"""
    rng = random.Random(T)
    jumped = 0
    for case in range(700):  # 2,100 cases over the three T
        L = rng.choice([1, 2, T - 1, T, T + 1, 2 * T + 1, 5 * T, 9 * T + 3])
        n_p = rng.choice([1, T - 1, T, T + 1, 3 * T + 2, rng.randrange(1, 12 * T)])
        kind = rng.randrange(4)
        if kind == 0:
            u = [1] * n_p
        elif kind == 1:
            u = [L] * n_p
        elif kind == 2:
            u = [rng.randrange(1, L + 1) for _ in range(n_p)]
        else:  # a run of 1-cell units, then L-cell units: the rows per tile change sharply
            u = [1] * (n_p // 2) + [L] * (n_p - n_p // 2)
        P = M.prefix(np.array(u, dtype=np.int64))
        plain, fill = [0], 0
        for k, x in enumerate(u):  # the sequential next-fit loop
            if fill + x > L:
                plain.append(k)
                fill = 0
            fill += x
        plain.append(n_p)
        assert M.row_starts(P, L).tolist() == plain
        starts, entered, tiles = M.rows_by_tiles(P, L, T)
        assert starts.tolist() == plain
        jumped += tiles - entered
    assert jumped > 0


@pytest.mark.parametrize("C", [4, 8])
def test_cells_by_tiles(C):
    """the write pass's narrowing of rows and pieces per tile of C cells gives every cell the model's piece"""
    rng = random.Random(C)
    for _ in range(400):
        ids, splits, L, bos, eos = random_case(rng)
        for mode, long_docs in ((M.NEXT_FIT, M.LONG_TRUNCATE), (M.NEXT_FIT, M.LONG_SPLIT), (M.STREAM, M.LONG_TRUNCATE)):
            out = M.pack(ids, splits, L, mode, bos, eos, 0, long_docs)
            if out["n_out"] == 0:
                continue
            doc, first, n, _ = M.pieces(splits, L, mode, bos, eos, long_docs)
            P = M.prefix(n + (bos >= 0) + (eos >= 0))
            starts = None if mode == M.STREAM else M.row_starts(P, L)
            piece, lengths, row_k0, row_seg = M.cells_by_tiles(P, int(P[-1]), L, out["n_out"], mode == M.STREAM, starts, C)
            assert lengths == out["lengths"].tolist()
            assert sum(row_seg) == out["stats"]["n_segments"]
            piece = piece.reshape(out["n_out"], L)
            seg = np.where(piece >= 0, 1 + piece - np.array(row_k0)[:, None], 0)
            assert np.array_equal(seg, out["segment_ids"])


def test_worked_examples():
    ids, splits = list(range(10, 17)), [0, 3, 3, 7]
    nf = M.pack(ids, splits, 4, M.NEXT_FIT, -1, 99, 0, M.LONG_TRUNCATE)
    assert nf["input_ids"].tolist() == [[10, 11, 12, 99], [13, 14, 15, 99]]
    assert (nf["stats"]["n_empty"], nf["stats"]["n_cut"], nf["stats"]["n_ids_cut"]) == (1, 1, 1)
    st = M.pack(ids, splits, 4, M.STREAM, -1, 99, 0)
    assert st["input_ids"].tolist() == [[10, 11, 12, 99], [13, 14, 15, 16], [99, 0, 0, 0]]
    assert st["lengths"].tolist() == [4, 4, 1] and st["segment_ids"][2].tolist() == [1, 0, 0, 0]
    assert st["source"][2].tolist() == [-1] * 4
    out = M.pack(list(range(6)), [0, 2, 5, 6], 8, M.NEXT_FIT, -1, 99, 0)  # units of 3, 4, 2 cells
    assert out["segment_ids"][0].tolist() == [1, 1, 1, 2, 2, 2, 2, 0]
    assert out["position_ids"][0].tolist() == [0, 1, 2, 0, 1, 2, 3, 0]
    assert out["n_out"] == 2 and out["lengths"].tolist() == [7, 2]
    none = M.pack([], [0, 0, 0], 4)
    assert none["n_out"] == 0 and none["input_ids"].shape == (0, 4) and none["stats"]["n_empty"] == 2
