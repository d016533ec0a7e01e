"""wp_pack_sequences / wp_pack_sequences_device on the GPU against the Python model (tests/pack_model.py): every block and
every statistic exactly.  The shapes sit at the kernels' edges (csrc/packing.h): T = kPackPieceTile pieces per tile of the
rows passes, C = kPackCellTile cells per tile of the write pass — units that fit exactly and by one cell not, rows that
end on a tile edge or jump over tiles, empty documents, long documents cut and split, rows and cells across tile
boundaries — not at workload size; one seeded case of 2 * 10^5 documents is checked against the same model."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pack_model as M
import wordpiece_amd as W

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")
T = 1024  # kPackPieceTile
CELLS = 2048  # kPackCellTile
VOCAB = ["[UNK]", "[CLS]", "[SEP]", "[PAD]", "[MASK]", "the", "cat", "sat", "on", "mat", "un", "##believ", "##able", "dog", "s", "##at"]
CLS, SEP, PAD = 1, 2, 3
SPECIALS = ((-1, -1), (-1, SEP), (CLS, SEP))  # none, eos only, bos + eos
ALL_MODES = (("next_fit", "truncate"), ("next_fit", "split"), ("stream", "truncate"))
KEYS = ("input_ids", "segment_ids", "position_ids", "source", "lengths")


def test_tile_sizes_match_the_kernels():
    src = open(os.path.join(PKG, "csrc", "packing.h")).read()
    block = int(re.search(r"constexpr int kBlock = (\d+);", open(os.path.join(PKG, "csrc", "common.h")).read()).group(1))
    items = {k: int(v) for k, v in re.findall(r"constexpr int (kPack\w+Items) = (\d+);", src)}
    assert re.search(r"kPackPieceTile = kBlock \* kPackPieceItems;", src) and re.search(r"kPackCellTile = kBlock \* kPackCellItems;", src)
    assert T == block * items["kPackPieceItems"] and CELLS == block * items["kPackCellItems"]
    assert 1 << int(re.search(r"constexpr int kPackLevels = (\d+);", src).group(1)) == T


@pytest.fixture(scope="module")
def gv():
    return W.Vocab(VOCAB)


def splits_of(lens):
    out = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(np.asarray(lens, dtype=np.int64), out=out[1:])
    return out


def ids_for(n):
    return (5 + np.arange(n, dtype=np.int64) * 7 % 1009).astype(np.int32)


def check(gv, lens, L, mode="next_fit", long_docs="truncate", bos=-1, eos=-1, pad=PAD):
    """the host entry point on documents of the lengths `lens` against the model: blocks and statistics"""
    splits = splits_of(lens)
    ids = ids_for(int(splits[-1]))
    exp = M.pack(ids, splits, L, M.MODES[mode], bos, eos, pad, M.LONG_DOCS[long_docs])
    got = gv.pack_sequences(ids, splits, max_len=L, mode=mode, bos_id=None if bos < 0 else bos, eos_id=None if eos < 0 else eos,
                            pad_id=pad, long_docs=long_docs)
    assert got["input_ids"].shape == (exp["n_out"], L), (got["input_ids"].shape, exp["n_out"], L)
    for k in KEYS:
        if not np.array_equal(got[k], exp[k]):
            bad = np.argwhere(got[k] != exp[k])[0]
            raise AssertionError("%s differs at %s: %d != %d (%d cells differ; L %d, %s, %s, bos %d, eos %d)" %
                                 (k, bad.tolist(), got[k][tuple(bad)], exp[k][tuple(bad)], int(np.sum(got[k] != exp[k])), L, mode,
                                  long_docs, bos, eos))
    assert gv.pack_stats() == exp["stats"]
    return exp


def fit_edges(gv):
    n = 0
    for bos, eos in SPECIALS:
        s = (bos >= 0) + (eos >= 0)
        L = 8
        B, m = L - s, 1  # m: the ids of the smallest unit
        for mode, long_docs in ALL_MODES:
            for lens in ([B, B, B],                       # units of exactly L
                         [B - m - s, m, B, B - m - s, m],  # L - (m + s) cells, then m + s: fits exactly
                         [B - m - s, m + 1, B - m - s, m + 1, 1]):  # ... then one cell more: does not
                check(gv, lens, L, mode, long_docs, bos, eos)
                n += 1
    for mode, long_docs in ALL_MODES:
        check(gv, [1, 3, 0, 1, 2], 1, mode, long_docs)            # L = 1 without specials
        check(gv, [1, 3, 0, 1, 2], 2, mode, long_docs, eos=SEP)   # L = 2 with one special: B = 1
        check(gv, [1, 3, 0, 1, 2], 2, mode, long_docs, bos=CLS)
        n += 3
    return n


def long_documents(gv):
    n = 0
    for bos, eos in SPECIALS:
        L = 9
        B = L - (bos >= 0) - (eos >= 0)
        for long_docs in ("truncate", "split"):
            for l in (B, B + 1, 2 * B, 2 * B + 1):
                check(gv, [2, l, 3, l], L, "next_fit", long_docs, bos, eos)
                n += 1
    return n


def stream_edges(gv):
    check(gv, [3, 5, 4], 4, "stream")                      # N = 12: no padding anywhere
    check(gv, [3, 5, 5], 4, "stream")                      # N = 13 = 3 L + 1
    check(gv, [4, 2], 4, "stream", eos=SEP)                # row 1 begins with the lone [SEP] of document 0
    exp = check(gv, [3, 0, 4], 4, "stream", eos=SEP, pad=0)  # the worked example
    assert exp["input_ids"][2].tolist() == [SEP, 0, 0, 0]
    check(gv, [2, 11, 1], 4, "stream", bos=CLS, eos=SEP)   # one unit over more than three rows
    return 5


def edge_grid(gv):
    """the small edge cases, for the release and for the bounds-checking build"""
    return fit_edges(gv) + long_documents(gv) + stream_edges(gv)


@pytest.mark.gpu
def test_fit_edges(gv):
    assert fit_edges(gv) == 36


@pytest.mark.gpu
def test_long_documents(gv):
    assert long_documents(gv) == 24
    for bos, eos in ((-1, SEP), (CLS, SEP)):
        B = 4 - (bos >= 0) - (eos >= 0)
        check(gv, [1, 3 * T * B + 1, 2], 4, "next_fit", "split", bos, eos)  # its pieces span tiles
        check(gv, [1, 3 * T * B + 1, 2], 4, "stream", bos=bos, eos=eos)
    check(gv, [3, 2 * 700 + 5, 1], 700, "stream", eos=SEP)  # l > 2 L: one unit over three rows


@pytest.mark.gpu
def test_stream_edges(gv):
    assert stream_edges(gv) == 5


@pytest.mark.gpu
@pytest.mark.parametrize("n_p", [T - 1, T, T + 1, 3 * T + 2])
def test_piece_tiles_mixed_units(gv, n_p):
    rng = np.random.default_rng(n_p)
    for L, eos in ((16, -1), (16, SEP), (5 * T // 2, SEP)):
        check(gv, rng.integers(1, min(L, 40) - (eos >= 0) + 1, n_p), L, eos=eos)


@pytest.mark.gpu
def test_piece_tiles_every_piece_a_row(gv):
    check(gv, [4] * (3 * T + 2), 4)            # T rows per tile
    check(gv, [3] * (2 * T + 1), 4, eos=SEP)
    check(gv, [7] * (T + 3), 4, long_docs="split")  # units of 4 and 3 cells in turn


@pytest.mark.gpu
@pytest.mark.parametrize("L", [T - 1, T, T + 1, 3 * T + 1])
def test_piece_tiles_one_cell_units(gv, L):
    """a row that ends on a tile edge (L = T), rows that start on a tile's last (T - 1) and first piece, rows that jump
    over one and over several tiles"""
    check(gv, [1] * (7 * T + 3), L)
    check(gv, [1] * (3 * L), L)  # the last row is full


@pytest.mark.gpu
def test_piece_tiles_rows_per_tile_change(gv):
    L = 64
    check(gv, [1] * (2 * T + 5) + [L] * (T + 7) + [1] * 70, L)
    check(gv, [L - 1] * (T + 7) + [1] * (2 * T + 5), L, eos=SEP)


@pytest.mark.gpu
def test_empty_documents(gv):
    some = [3, 1, 4, 1, 5, 9, 2, 6]
    between = [x for l in some for x in (l, 0)][:-1]
    for mode, long_docs in ALL_MODES:
        for lens in ([0, 0] + some, some + [0, 0, 0], some[:3] + [0] * (T + 9) + some[3:], between, [0] * (T + 2) + [1]):
            check(gv, lens, 8, mode, long_docs, eos=SEP)
        exp = check(gv, [0] * 5, 8, mode, long_docs, eos=SEP)
        assert exp["n_out"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("L", [5, 127, 128, 129])
def test_cell_tiles_rows_across(gv, L):
    rng = np.random.default_rng(L)
    lens = rng.integers(1, L, 3 * CELLS // (L // 2) + 8)  # enough rows to cross 3 C cells
    for mode, long_docs in ALL_MODES:
        exp = check(gv, lens, L, mode, long_docs, eos=SEP)
        assert exp["n_out"] * L > 3 * CELLS


@pytest.mark.gpu
def test_cell_tiles_exact_sizes(gv):
    for L, rows in ((89, 23), (128, 16), (683, 3)):  # n_out * L = C - 1, C, C + 1
        assert L * rows in (CELLS - 1, CELLS, CELLS + 1)
        for mode in ("next_fit", "stream"):
            exp = check(gv, [L] * rows, L, mode)
            assert exp["n_out"] == rows
        check(gv, [L - 2, 1] * (rows - 1) + [3], L, "next_fit", eos=SEP)
    exp = check(gv, [CELLS, CELLS, 5], 3 * CELLS + 2)  # a single row of more than three tiles
    assert exp["n_out"] == 1
    check(gv, [CELLS, CELLS, 5], 3 * CELLS + 2, "stream", bos=CLS)
    check(gv, [1] * (2 * CELLS + 7), 3 * CELLS + 2, eos=SEP)  # ... of more pieces than a tile has cells


def tensor_call(gv, ids, splits, L, spec_kw, cap, fill=-77):
    """the device entry point on sentinel-filled buffers of cap rows -> (rc, n_out, buffers as numpy)"""
    import torch
    dev = torch.device("cuda")
    d_ids = torch.as_tensor(np.asarray(ids, np.int32), device=dev)
    d_splits = torch.as_tensor(np.asarray(splits, np.int64), device=dev)
    bufs = {k: torch.full((cap,) if k == "lengths" else (cap, L), fill, dtype=torch.int32, device=dev) for k in KEYS}
    spec = W.PackSpec(max_len=L, mode=0, bos_id=-1, eos_id=-1, pad_id=PAD, long_docs=0, want=7)
    for k, v in spec_kw.items():
        setattr(spec, k, v)
    n = C.c_size_t()
    torch.cuda.synchronize()
    rc = W.lib().wp_pack_sequences_device(gv._h, C.c_void_p(d_ids.data_ptr()), C.c_void_p(d_splits.data_ptr()), len(splits) - 1,
                                          C.byref(spec), C.byref(W.Packed(*[bufs[k].data_ptr() for k in KEYS])), cap, C.byref(n))
    return rc, n.value, {k: v.cpu().numpy() for k, v in bufs.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("want", range(8))
def test_want(gv, want):
    lens = [3, 0, 6, 2, 9, 1]
    splits, L = splits_of(lens), 8
    ids = ids_for(int(splits[-1]))
    for mode in (M.NEXT_FIT, M.STREAM):
        exp = M.pack(ids, splits, L, mode, CLS, SEP, PAD, M.LONG_SPLIT, want)
        rc, n_out, got = tensor_call(gv, ids, splits, L, dict(mode=mode, bos_id=CLS, eos_id=SEP, long_docs=1, want=want), exp["n_out"] + 2)
        assert rc == 0 and n_out == exp["n_out"]
        for k, bit in (("input_ids", 0), ("segment_ids", 1), ("position_ids", 2), ("source", 4), ("lengths", 0)):
            if bit == 0 or want & bit:
                assert np.array_equal(got[k][:n_out], exp[k]), k
                assert np.all(got[k][n_out:] == -77), k  # rows behind n_out untouched
            else:
                assert exp[k] is None and np.all(got[k] == -77), k  # an unwanted output keeps the sentinel
        # the Python mirrors return the wanted blocks only
        names = [k for k, bit in W._PACK_WANT.items() if want & bit]
        out = gv.pack_sequences(ids, splits, max_len=L, mode=("next_fit", "stream")[mode], bos_id=CLS, eos_id=SEP, pad_id=PAD,
                                long_docs="split", want=names)
        assert sorted(out) == sorted(["input_ids", "lengths"] + names)
        assert all(np.array_equal(out[k], exp[k]) for k in out)
        assert gv.pack_stats() == exp["stats"]


@pytest.mark.gpu
def test_capacity_and_bad_row_splits(gv):
    L = W.lib()
    lens = [5, 7, 3, 8, 8, 1, 2]
    splits = splits_of(lens)
    ids = ids_for(int(splits[-1]))
    for mode in (M.NEXT_FIT, M.STREAM):
        exp = M.pack(ids, splits, 8, mode, -1, SEP, PAD)
        rc, n_out, got = tensor_call(gv, ids, splits, 8, dict(mode=mode, eos_id=SEP), exp["n_out"] - 1)
        assert rc == 6 and b"capacity_rows" in L.wp_last_error() and n_out == exp["n_out"]
        assert all(np.all(x == -77) for x in got.values())
        rc, n_out, got = tensor_call(gv, ids, splits, 8, dict(mode=mode, eos_id=SEP), exp["n_out"] + 3)
        assert rc == 0 and n_out == exp["n_out"] and all(np.all(got[k][n_out:] == -77) for k in KEYS)
        assert all(np.array_equal(got[k][:n_out], exp[k]) for k in KEYS)
        for bad in (splits + 1, np.concatenate([splits[:3], [splits[2] - 1], splits[4:]])):  # row_splits[0] != 0; a descent
            rc, n_out, got = tensor_call(gv, ids, bad, 8, dict(mode=mode, eos_id=SEP), 16)
            assert rc == 6 and b"row_splits must" in L.wp_last_error() and n_out == 0
            assert all(np.all(x == -77) for x in got.values())
    # the tensor mirror sizes its own buffers, and asks again where split mode needs more rows than documents
    import torch
    out = gv.pack_sequences_tensor(torch.as_tensor(ids, device="cuda"), torch.as_tensor(splits, device="cuda"), max_len=4, eos_id=SEP,
                                   long_docs="split")
    exp = M.pack(ids, splits, 4, M.NEXT_FIT, -1, SEP, 0, M.LONG_SPLIT)
    assert exp["n_out"] > len(lens) and all(np.array_equal(out[k].cpu().numpy(), exp[k]) for k in KEYS)


@pytest.mark.gpu
def test_composition_with_rows_word_ids_and_detokenize(gv):
    """text -> rows -> packed batch -> word ids, text and offsets, nothing leaving the device in between"""
    import torch
    docs = ["the cat sat on the mat", "unbelievable", "", "the dog sat", "sat", "on the mat the cat sat on", "dog"]
    text, off = W.join_docs(docs)
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    d_off = torch.as_tensor(np.asarray(off, np.int64)).cuda()
    ids, splits, offs = gv.encode_rows_tensor(d_text, d_off, offsets="byte", copy=False)  # (views: the pack has buffers of its own)
    L = 12
    out = gv.pack_sequences_tensor(ids, splits, max_len=L, bos_id=CLS, eos_id=SEP, pad_id=PAD)
    # offsets: one gather carries them into the batch (the rows result is still there behind the pack)
    gathered = offs.view(torch.int32)[out["source"].clamp(min=0).long()].cpu().numpy().view(np.uint32)
    h_ids, h_splits, h_offs = ids.cpu().numpy(), splits.cpu().numpy(), offs.cpu().numpy()
    assert np.array_equal(h_ids, gv.encode_rows(docs)[0])  # the rows result survived the pack
    exp = M.pack(h_ids, h_splits, L, M.NEXT_FIT, CLS, SEP, PAD)
    assert exp["stats"]["n_cut"] == 0 and exp["n_out"] >= 3
    assert all(np.array_equal(out[k].cpu().numpy(), exp[k]) for k in KEYS)
    same = gv.encode_packed_tensor(d_text, d_off, max_len=L, bos_id=CLS, eos_id=SEP, pad_id=PAD)
    assert all(torch.equal(same[k], out[k]) for k in KEYS)
    # word ids: per document, a token that is no "##" continuation begins a word; laid out through the model's source
    word = np.zeros(len(h_ids), np.int32)
    for a, b in zip(h_splits[:-1], h_splits[1:]):
        w = -1
        for i in range(a, b):
            w += 0 if VOCAB[h_ids[i]].startswith("##") else 1
            word[i] = w
    src = exp["source"]
    got = gv.word_ids_tensor(out["input_ids"], out["lengths"], cls_id=CLS, sep_id=SEP, pad_id=PAD).cpu().numpy()
    assert np.array_equal(got, np.where(src >= 0, word[np.maximum(src, 0)], -1))
    # text: the documents of a row, in order
    t, t_off = gv.detokenize_tensor(out["input_ids"], lengths=out["lengths"], skip_ids=[CLS, SEP, PAD])
    t, t_off = bytes(t.cpu().numpy()), t_off.cpu().numpy()
    doc_of = np.searchsorted(h_splits, np.arange(len(h_ids)), side="right") - 1
    for r in range(exp["n_out"]):
        in_row = sorted(set(doc_of[src[r][src[r] >= 0]].tolist()))
        assert t[t_off[r]:t_off[r + 1]].decode() == " ".join(docs[d] for d in in_row)
    assert np.array_equal(gathered[src >= 0], h_offs[src[src >= 0]])


@pytest.mark.gpu
@pytest.mark.parametrize("L", [128, 512])
def test_at_size(gv, L):
    rng = np.random.default_rng(2024)
    lens = np.minimum(rng.lognormal(2.3, 1.1, 200_000).astype(np.int64), 4000)  # long-tailed: median 10, many empty, some > L
    for mode, long_docs in (("next_fit", "truncate"), ("stream", "truncate")):
        exp = check(gv, lens, L, mode, long_docs, bos=CLS, eos=SEP)
        assert exp["stats"]["n_empty"] > 0 and exp["n_out"] > 10 * T // 4


@pytest.mark.gpu
def test_bounds_checking_build(tmp_path):
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "pack_dbg_run.py"
    script.write_text('''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import wordpiece_amd as W
from test_gpu_pack import VOCAB, T, edge_grid, check
gv = W.Vocab(VOCAB)
gv.encode("the cat")
assert gv.stats()["reserved0"] == 1, "not the bounds-checking build"
assert edge_grid(gv) == 65
check(gv, [1] * (3 * T + 5), T + 1, eos=2)
check(gv, [5] * (2 * T + 1), 9, "stream", eos=2)
print("PACK_DEBUG_OK")
''' % (os.path.dirname(PKG), HERE))
    env = dict(os.environ, WP_LIB=dbg)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "PACK_DEBUG_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
