"""GPU checks of the near-duplicate clustering (wp_neardup_rows, wp_neardup_rows_device) against tests/neardup_model.py,
exactly: every output array with its dtype, every signature entry, the compact form and the statistics the contract
fixes — at the tile and segment edges of the signature kernel, at every shingle and permutation shape, with one long row
beside short ones, on components that are no stars, where min_agree decides, on duplicates and empties, with bytes
behind the data, with bad offsets, across the states of a handle and end to end with the encoder, the packer and the
detokenizer."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import neardup_model as M
import wordpiece_amd as W

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")
VOCAB = ["[UNK]", "a", "b", "##b", "中", "."]
T = 1024        # shingle positions per workgroup of the signature kernel (neardup.h: kNearTile)
SEG = T // 4    # positions a wave walks (neardup.h: kNearSeg)
STAT_KEYS = ("n_rows", "n_unique", "n_empty", "n_elems", "n_shingles", "n_buckets", "n_candidates", "n_edges")


def test_geometry_matches_the_kernels():
    src = open(os.path.join(PKG, "csrc", "neardup.h")).read()
    common = open(os.path.join(PKG, "csrc", "common.h")).read()
    block = int(re.search(r"constexpr int kBlock = (\d+);", common).group(1))
    wave = int(re.search(r"constexpr int kWave = (\d+);", common).group(1))
    assert int(re.search(r"constexpr int kNearTile = (\d+);", src).group(1)) == T
    assert re.search(r"constexpr int kNearSeg = kNearTile / \(kBlock / kWave\);", src) and T // (block // wave) == SEG
    assert re.search(r"constexpr int kNearMaxShingle = 64;", src) and re.search(r"constexpr int kNearMaxPerm = 256;", src)
    assert re.search(r"kSiteNearDup = 18,", common)


_handle = []


def handle():
    if not _handle:
        _handle.append(W.Vocab(VOCAB))
    return _handle[0]


def to_gpu(data, eb):
    import torch
    dtype = torch.uint8 if eb == 1 else torch.int32
    if not data:
        return torch.zeros(0, dtype=dtype, device="cuda")
    return torch.frombuffer(bytearray(data), dtype=dtype).cuda()


def compare(got, exp, eb, where, tensor):
    """every array of one call against the model's, dtype included"""
    if tensor:
        got = {k: x.cpu().numpy() for k, x in got.items()}
        assert got["signatures"].dtype == np.int32  # (the bit patterns: see neardup_rows_tensor)
        got["signatures"] = got["signatures"].view(np.uint32)
    for key, dtype in (("cluster", np.int32), ("kept", np.int32), ("counts", np.int64), ("inverse", np.int32), ("row_off", np.int64)):
        assert got[key].dtype == dtype and got[key].tolist() == exp[key], (where, key)
    assert got["data"].dtype == (np.uint8 if eb == 1 else np.int32) and got["data"].tobytes() == exp["data"], (where, "data")
    sig = got["signatures"]
    assert sig.dtype == np.uint32 and sig.shape == exp["signatures"].shape, (where, "signatures")
    if not np.array_equal(sig, exp["signatures"]):
        bad = np.argwhere(sig != exp["signatures"])
        raise AssertionError((where, "signatures", len(bad), bad[:5].tolist()))


def check(rows, where, eb=1, forms=(False, True), v=None, **spec):
    """the rows (bytes each) through the host form and the tensor form against the model; -> (the model's answer, the
    statistics of the last call)"""
    import torch
    v = v or handle()
    data, off = M.join(rows, eb)
    exp = M.neardup_rows(data, off, eb, **spec)
    st = None
    for tensor in forms:
        if tensor:
            got = v.neardup_rows_tensor(to_gpu(data, eb), torch.tensor(off, dtype=torch.int64, device="cuda"), inverse=True, compact=True,
                                        signatures=True, **spec)
        else:
            got = v.neardup_rows(np.frombuffer(data, dtype=np.uint8 if eb == 1 else np.int32), off, inverse=True, compact=True, signatures=True,
                                 raw=True, **spec)
        compare(got, exp, eb, (where, "tensor" if tensor else "host"), tensor)
        st = v.neardup_stats()
        assert {k: st[k] for k in STAT_KEYS} == exp["stats"], (where, st, exp["stats"])
        assert (st["n_rounds"] >= 1) == (exp["stats"]["n_edges"] > 0), where
    return exp, st


def random_row(rng, n_elems, eb, alphabet=6):
    """n_elems elements over a small alphabet: rows of the same length share many shingles"""
    if eb == 1:
        return bytes(rng.integers(97, 97 + alphabet, n_elems, dtype=np.uint8))
    return rng.integers(1000, 1000 + alphabet, n_elems, dtype=np.int32).tobytes()


def rows_of_positions(rng, positions, k, eb, alphabet=6):
    """a row of p shingle positions has p + k - 1 elements (p >= 1)"""
    return [random_row(rng, p + k - 1, eb, alphabet) for p in positions]


@pytest.mark.gpu
@pytest.mark.parametrize("eb", [1, 4])
def test_rows_at_the_tile_and_segment_edges(eb):
    rng = np.random.default_rng(3 + eb)
    k = 5
    spec = dict(shingle=k, n_perm=128, bands=16)
    # the first row's positions end 1 before, on and 1 after a segment edge and a tile edge
    for edge in (SEG, T):
        for first in (edge - 1, edge, edge + 1):
            rows = rows_of_positions(rng, [first, 3, 1, 1, SEG - 2, 2, 1], k, eb)
            rows += [rows[0], rows[3]]
            check(rows, ("edge", edge, first), eb, **spec)
    # rows that span 2 and 3 tiles (atomicMin from several workgroups) beside rows of 1 position
    rows = rows_of_positions(rng, [1, 1, 2 * T + 5, 1, 1, T + 3, 1, 1], k, eb)
    exp, _ = check(rows, "spanning rows", eb, **spec)
    assert exp["stats"]["n_shingles"] == 3 * T + 14
    # a row that starts on the last position of a tile, and one that starts on the last position of a segment
    check(rows_of_positions(rng, [T - 1, 7, 2], k, eb), "starts on the last position of a tile", eb, **spec)
    check(rows_of_positions(rng, [SEG - 1, SEG + 9, 2], k, eb), "starts on the last position of a segment", eb, **spec)
    # exactly one tile, and one position more
    check(rows_of_positions(rng, [T // 2, T // 2], k, eb), "one full tile", eb, **spec)
    check(rows_of_positions(rng, [T // 2, T // 2, 1], k, eb), "one full tile and one", eb, **spec)


@pytest.mark.gpu
def test_text_rows_at_every_byte_alignment():
    rng = np.random.default_rng(5)
    base = [random_row(rng, n, 1) for n in (1, 4, 5, 9, 12, 13, 40)]
    for lead in (0, 1, 2, 3):
        rows = ([b"\xee" * lead] if lead else []) + base + base[::-1]
        exp, _ = check(rows, ("lead", lead), 1, shingle=5, n_perm=64, bands=8)
        assert exp["stats"]["n_unique"] <= len(base) + 1
    # one row placed four times, each copy at another offset mod 4: all four are one cluster with one signature
    for n in (3, 8, 21):
        row, rows, total = random_row(rng, n, 1, 20), [], 0
        for c in range(4):
            if c:
                pad = (c - total) % 4 or 4
                rows.append(b"\xee" * pad)
                total += pad
            assert total % 4 == c
            rows.append(row)
            total += n
        exp, _ = check(rows, ("placed", n), 1, shingle=8, n_perm=16, bands=4, min_agree=16)
        assert exp["counts"][0] == 4, n


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 5, 8, 9, 64])
def test_shingle_lengths_and_row_lengths(k):
    rng = np.random.default_rng(k)
    for eb in (1, 4):
        lengths = sorted({0, 1, max(k - 1, 0), k, k + 1, 2 * k + 3, 100})
        rows = [random_row(rng, n, eb, 4) for n in lengths for _ in range(2)]
        rows += [rows[-1], rows[2], b""]
        exp, _ = check(rows, ("k", k, eb), eb, shingle=k, n_perm=32, bands=8)
        assert exp["stats"]["n_empty"] == 3 and exp["stats"]["n_shingles"] == sum(max(len(r) // eb - k + 1, 1) for r in rows if r)


def near_duplicate_batch(rng, eb, n_docs=12, n_rows=40):
    docs = [random_row(rng, int(rng.integers(20, 60)), eb, 30) for _ in range(n_docs)]
    rows = []
    for _ in range(n_rows):
        row = bytearray(docs[int(rng.integers(n_docs))])
        for _ in range(int(rng.integers(0, 3))):
            at = int(rng.integers(len(row) // eb)) * eb
            row[at] ^= 0x15
        rows.append(bytes(row))
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("n_perm", [1, 16, 63, 64, 65, 96, 128, 256])
def test_permutation_and_band_shapes(n_perm):
    proper = {1: 1, 16: 4, 63: 9, 64: 16, 65: 13, 96: 24, 128: 32, 256: 64}[n_perm]
    for eb in (1, 4):
        rows = near_duplicate_batch(np.random.default_rng(n_perm + eb), eb)
        for bands in sorted({1, proper, n_perm}):
            for min_agree in (0, n_perm // 2):
                check(rows, ("n_perm", n_perm, bands, min_agree, eb), eb, forms=(bands == proper,), shingle=3, n_perm=n_perm, bands=bands,
                      min_agree=min_agree, seed=n_perm * 1000003)


@pytest.mark.gpu
def test_one_long_row_beside_short_ones():
    rng = np.random.default_rng(4)
    long = rng.integers(0, 256, 300_000, dtype=np.uint8).tobytes()
    short = [bytes(rng.integers(97, 101, 10, dtype=np.uint8)) for _ in range(1000)]
    rows = short[:300] + [long] + short[300:]
    exp, st = check(rows, "long row", 1)
    assert exp["stats"]["n_shingles"] == 300_000 - 4 + 1000 * 6 and exp["cluster"][300] == 300
    ids = rng.integers(0, 30000, 300_000, dtype=np.int32).tobytes()
    short = [rng.integers(5, 9, 10, dtype=np.int32).tobytes() for _ in range(1000)]
    check(short[:700] + [ids] + short[700:] + [ids], "long id row", 4, forms=(True,))


@pytest.mark.gpu
def test_components_that_are_not_stars():
    rng = random.Random(9)
    xs = rng.sample(range(1, 10 ** 6), 201)
    order = list(range(200))
    rng.shuffle(order)  # row order[p] holds {x_p, x_p+1}: the row indices are shuffled along the chain
    rows = [None] * 200
    for p, i in enumerate(order):
        rows[i] = np.array([xs[p], xs[p + 1]], dtype=np.int32).tobytes()
    exp, st = check(rows, "chain, 32 bands", 4, shingle=1, n_perm=32, bands=32, min_agree=0)
    # (asserted on the model) one cluster, and not a star: some row has no edge to the cluster's row
    assert exp["cluster"] == [0] * 200 and exp["kept"] == [0] and exp["counts"] == [200]
    assert any((i, 0) not in exp["edges"] for i in range(1, 200))
    exp16, _ = check(rows, "chain, 16 bands", 4, shingle=1, n_perm=16, bands=16, min_agree=0)
    assert sum(exp16["counts"]) == 200
    # two chains in one batch, and a ring
    more = rows + [np.array([xs[p] + 10 ** 7, xs[p + 1] + 10 ** 7], dtype=np.int32).tobytes() for p in range(100)]
    more.append(np.array([xs[100] + 10 ** 7, xs[0] + 10 ** 7], dtype=np.int32).tobytes())
    exp2, _ = check(more, "two components", 4, shingle=1, n_perm=32, bands=32, min_agree=0)
    assert len(exp2["kept"]) >= 2


@pytest.mark.gpu
def test_min_agree_decides():
    line = b"the quick brown fox jumps over the lazy dog while the cat sleeps under a warm yellow sun today ok"[:96]
    v1, v2 = line.replace(b"brown", b"black"), line.replace(b"yellow", b"orange!")[:96]
    other = bytes(reversed(b"pack my box with five dozen liquor jugs and then send it over to the other side of the town ok!!"))[:96]
    rows = [line, v1, v2, other]
    spec = dict(shingle=5, n_perm=128, bands=32)
    exp, _ = check(rows, "min_agree 64", 1, min_agree=W.lsh_min_agree(0.5, 128), **spec)
    sig = exp["signatures"]
    agree = [int((sig[i] == sig[0]).sum()) for i in range(4)]
    assert agree[0] == 128 and min(agree[1:3]) >= 64 and agree[1] != agree[2] and agree[3] < 64  # (the model: 108, 103, 0)
    assert exp["cluster"] == [0, 0, 0, 3]
    # a threshold between the two variants: both are compared with the head, one passes
    between = max(agree[1:3])
    exp, _ = check(rows, "min_agree between", 1, min_agree=between, **spec)
    assert exp["stats"]["n_candidates"] > exp["stats"]["n_edges"] > 0 and sorted(exp["counts"]) == [1, 1, 2]
    exp, _ = check(rows, "min_agree 0", 1, min_agree=0, **spec)
    assert exp["stats"]["n_candidates"] == exp["stats"]["n_edges"] and exp["cluster"] == [0, 0, 0, 3]
    exp, _ = check(rows + [line], "min_agree n_perm", 1, min_agree=128, **spec)
    assert exp["cluster"] == [0, 1, 2, 3, 0]


@pytest.mark.gpu
def test_exact_duplicates_and_empties():
    rng = np.random.default_rng(8)
    for eb in (1, 4):
        a, b, short = random_row(rng, 50, eb, 40), random_row(rng, 70, eb, 40), random_row(rng, 3, eb, 40)
        rows = [b"", a, short, b"", b, a, short, b"", b, a, b""]
        exp, _ = check(rows, ("duplicates", eb), eb, shingle=5, n_perm=64, bands=8, min_agree=64)
        # equal rows share a cluster, shorter than a shingle too; empty rows are each their own (unlike dedup_rows)
        assert exp["cluster"] == [0, 1, 2, 3, 4, 1, 2, 7, 4, 1, 10]
    import torch
    v = handle()
    # all rows empty in the device form (the host form answers without a device)
    for n in (1, 5, 3000):
        got = v.neardup_rows_tensor(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(n + 1, dtype=torch.int64, device="cuda"),
                                    n_perm=4, bands=2, inverse=True, compact=True, signatures=True)
        compare(got, M.neardup_rows(b"", [0] * (n + 1), n_perm=4, bands=2), 1, ("all empty", n), True)
        st = v.neardup_stats()
        assert (st["n_rows"], st["n_unique"], st["n_empty"], st["n_shingles"], st["n_edges"], st["n_rounds"]) == (n, n, n, 0, 0, 0)
    got = v.neardup_rows_tensor(torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), compact=True)
    assert got["cluster"].numel() == 0 and got["kept"].numel() == 0 and got["row_off"].tolist() == [0] and v.neardup_stats()["n_rows"] == 0
    # a hot bucket: many copies of one line, every band of every copy in the head's bucket
    n = 20_000
    row = b"the same line\n"
    off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * len(row)
    got = v.neardup_rows_tensor(to_gpu(row * n, 1), off, inverse=True, compact=True, min_agree=128)
    assert not got["cluster"].any() and got["kept"].tolist() == [0] and got["counts"].tolist() == [n]
    assert got["data"].cpu().numpy().tobytes() == row and got["row_off"].tolist() == [0, len(row)]
    st = v.neardup_stats()
    assert (st["n_unique"], st["n_buckets"], st["n_candidates"], st["n_edges"]) == (1, 16, 16 * (n - 1), 16 * (n - 1))
    # the documents form and the lines form, through the host call
    docs = ["the cat sat on the mat today", "a", "the cat sat on the mat today!", "", "a", "something else entirely here"]
    kept, counts = v.neardup_docs(docs, min_agree=W.lsh_min_agree(0.5, 128))
    exp = M.neardup_rows(*W.join_docs(docs), min_agree=64)
    assert kept == [docs[i] for i in exp["kept"]] and counts.tolist() == exp["counts"] and exp["cluster"][:3] == [0, 1, 0] and exp["cluster"][4] == 1
    r = v.neardup_rows(b"x y z w v\nq\nx y z w v\n\nx y z w v", compact=True)  # (the last line gets its line feed)
    assert r["kept"].tolist() == [0, 1, 3] and r["counts"].tolist() == [3, 1, 1] and r["data"] == b"x y z w v\nq\n\n"


@pytest.mark.gpu
def test_bytes_behind_the_data_are_not_read():
    import torch
    v = handle()
    rng = np.random.default_rng(12)
    rows = [random_row(rng, 301, 1), b"ab", random_row(rng, 40, 1), b"ab", random_row(rng, 5, 1), b"abc"]
    data, off = M.join(rows)
    assert len(data) % 4 != 0
    exp = M.neardup_rows(data, off)
    off_t = torch.tensor(off, dtype=torch.int64, device="cuda")
    for fill in (0x00, 0xff, 0x61):
        big = torch.full((len(data) + 4096,), fill, dtype=torch.uint8, device="cuda")
        big[:len(data)] = to_gpu(data, 1)
        view = big[:(len(data) + 259) // 4 * 4]  # a prefix view that is aligned and whole words long: it is passed as it is
        assert view.data_ptr() == big.data_ptr() and view.numel() > len(data)
        compare(v.neardup_rows_tensor(view, off_t, inverse=True, compact=True, signatures=True), exp, 1, ("trailing", fill), True)
        assert v.neardup_stats()["n_elems"] == len(data)
    # a text whose last row ends on the last byte of its tensor, at every length mod 4
    for extra in range(4):
        rows2 = rows + [b"z" * extra, b"abc"]
        check(rows2, ("last byte", extra), 1, forms=(True,))
    # ids behind the last row
    ids = np.array([3, 4, 3, 4, 9, 9, 9], dtype=np.int32)
    got = v.neardup_rows_tensor(torch.from_numpy(ids).cuda(), torch.tensor([0, 2, 4], dtype=torch.int64, device="cuda"), shingle=2, compact=True)
    assert got["cluster"].tolist() == [0, 0] and got["data"].tolist() == [3, 4] and v.neardup_stats()["n_elems"] == 4


@pytest.mark.gpu
def test_bad_offsets_in_the_device_form():
    import torch
    v = W.Vocab(VOCAB)
    data = to_gpu(b"abcdefghijklmnop", 1)
    good = [0, 2, 4, 6, 8, 10, 12]
    for bad_row, off in ((0, [0, -1, 4, 6, 8, 10, 12]), (0, [1, 2, 4, 6, 8, 10, 12]), (3, [0, 2, 4, 7, 6, 10, 12]), (5, [0, 2, 4, 6, 8, 10, 9]),
                         (1, [0, 5, 4, 3, 8, 10, 12]), (2, [0, 2, 2 ** 40, 6, 8, 10, 12])):
        with pytest.raises(W.WordPieceError, match=r"row_off must .* row %d$" % bad_row):
            v.neardup_rows_tensor(data, torch.tensor(off, dtype=torch.int64, device="cuda"))
        got = v.neardup_rows_tensor(data, torch.tensor(good, dtype=torch.int64, device="cuda"))  # the handle is usable afterwards
        assert got["cluster"].tolist() == list(range(6)) and v.neardup_stats()["n_unique"] == 6
    with pytest.raises(W.WordPieceError, match="UINT32_MAX"):
        v.neardup_rows_tensor(data, torch.tensor([0, 2, 2 ** 33], dtype=torch.int64, device="cuda"))
    assert v.encode("ab a").tolist() == [1, 3, 1]


@pytest.mark.gpu
def test_handle_state():
    import torch
    import dedup_model as DM
    v = W.Vocab(VOCAB)
    assert v.neardup_stats()["n_rows"] == -1
    rng = np.random.default_rng(14)
    small = [b"ab ab ab", b"a", b"ab ab ab"]
    large = near_duplicate_batch(rng, 1, n_docs=60, n_rows=2000)
    check(small, "first call", v=v)
    text = ("b a b . 中 ab a b " * 40).encode("utf8")
    ids = v.encode(text)
    assert len(ids) == 9 * 40 and v.neardup_stats()["n_rows"] == -1  # (an encode since: as every layer's statistics)
    check(large, "grown", v=v, forms=(True,))
    assert v.dedup_stats()["n_rows"] == -1
    d = v.dedup_rows(*DM.join(large), compact=True)
    assert d["kept"].tolist() == DM.dedup_rows(*DM.join(large))["kept"] and v.neardup_stats()["n_rows"] == 2000  # (each layer keeps its own)
    words = v.count_words(text)
    assert words["counts"].sum() == 8 * 40
    check(small + [b""], "shrunk, behind a dedup and a count call", v=v, forms=(True,))
    assert v.encode(text).tolist() == ids.tolist() and v.neardup_stats()["n_rows"] == -1
    # views live until the handle's next call, whatever other handles do
    data, off = M.join(large)
    dt, ot = to_gpu(data, 1), torch.tensor(off, dtype=torch.int64, device="cuda")
    views = v.neardup_rows_tensor(dt, ot, inverse=True, compact=True, signatures=True, copy=False)
    kept = {k: x.clone() for k, x in views.items()}
    other = W.Vocab(["x", "b a"])
    other.neardup_rows_tensor(dt[:ot[40]], ot[:41], inverse=True, compact=True, signatures=True)
    other.encode(text)
    assert all(torch.equal(views[k], kept[k]) for k in views)
    copies = v.neardup_rows_tensor(dt, ot, inverse=True, compact=True, signatures=True)
    assert all(torch.equal(copies[k], kept[k]) for k in kept)
    for rows, trim in ((small, False), (large[:700], False), ([b"q"], True), (large[:90], False)):
        if trim:
            v.trim()
        check(rows, ("sizes", len(rows), trim), v=v, forms=(trim,))


@pytest.mark.gpu
def test_end_to_end_with_the_encoder_the_packer_and_the_detokenizer():
    import torch
    import normalize_model as NM
    import oracle_lib as O
    vocab = ["[UNK]", "[CLS]", "[SEP]", "hello", "world", ",", "cafe", "##s", "a", "b", "the", "##x", "of", "and", "is", "in"]
    page = "the world of cafes is in the world and hello is a cafe of the b and the a , hello world "
    docs = [page, page.upper(), page.replace("hello world ", "hello , world "), "cafés", "the a b", page.replace("  ", " ") + "in",
            "", "CAFES", "a b " * 60, "A  B " * 60 + "a", "world hello"]
    v = W.Vocab(vocab, normalize=W.WP_NORM_BERT_UNCASED)
    oracle = O.Vocab(vocab)
    want_ids = [np.asarray(oracle.encode(NM.normalize(d.encode("utf8"), W.WP_NORM_BERT_UNCASED)[0]), dtype=np.int32) for d in docs]
    spec = dict(shingle=5, n_perm=128, bands=16, min_agree=W.lsh_min_agree(0.6, 128))
    exp = M.neardup_rows(*M.join([w.tobytes() for w in want_ids], 4), elem_bytes=4, **spec)
    text, off = W.join_docs(docs)
    t = torch.zeros((len(text) + 19) // 16 * 16, dtype=torch.uint8, device="cuda")
    t[:len(text)] = to_gpu(text, 1)
    ids, splits = v.encode_rows_tensor(t[:len(text)], torch.from_numpy(off).cuda())
    got = v.neardup_rows_tensor(ids, splits, inverse=True, compact=True, signatures=True, **spec)
    compare(got, exp, 4, "ids of the rows call", True)
    # the page, its upper-case copy and its two edits are one document; so are the two runs of "a b"; the empty row is alone
    assert exp["cluster"][:3] == [0, 0, 0] and exp["cluster"][5] == 0 and exp["cluster"][7] == 3 and exp["cluster"][9] == 8 and exp["cluster"][6] == 6
    # the compact form is what the packer takes; its rows, detokenized, are the model's kept documents
    packed = v.pack_sequences_tensor(got["data"], got["row_off"], max_len=512)
    texts = v.detokenize(got["data"].cpu().numpy(), row_splits=got["row_off"].cpu().numpy())
    model_kept = [" ".join(NM.normalize(docs[i].encode("utf8"), W.WP_NORM_BERT_UNCASED)[0].decode("utf8").split()).replace(" ,", ",")
                  for i in exp["kept"]]
    assert exp["kept"] == [0, 3, 4, 6, 8, 10] and texts == model_kept and texts[1:4] == ["cafes", "the a b", ""]
    flat = np.frombuffer(exp["data"], dtype=np.int32)
    assert int(packed["lengths"].sum()) == flat.size


@pytest.mark.gpu
@pytest.mark.parametrize("lib_name,guard", [("libwordpiece_amd_dbg.so", "0"), ("libwordpiece_amd.so", "1")])
def test_hardened_runs(tmp_path, lib_name, guard):
    """(a fresh child: once on the bounds-checking build, once with WP_ARENA_GUARD=1) the tile-edge, the chain and the
    long-row cases: no gather or store outside an array (kSiteNearDup, kSiteGroup), no guard zone of the call's
    arenas overwritten"""
    lib = os.path.join(PKG, lib_name)
    assert os.path.exists(lib), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "neardup_hard_run.py"
    script.write_text('''
import sys
import torch  # (before the library, as tests/conftest.py: the HIP runtime loaded first serves the process)
sys.path.insert(0, %r); sys.path.insert(0, %r)
import wordpiece_amd as W
import test_gpu_neardup as T
v = T.handle()
v.encode("ab a")
assert v.stats()["reserved0"] == %d, "not the build this run is about"
T.test_rows_at_the_tile_and_segment_edges(1)
T.test_rows_at_the_tile_and_segment_edges(4)
T.test_components_that_are_not_stars()
T.test_one_long_row_beside_short_ones()
print("NEARDUP_HARD_OK")
''' % (os.path.dirname(PKG), HERE, 1 if "dbg" in lib_name else 0))
    env = dict(os.environ, WP_LIB=lib, WP_ARENA_GUARD=guard)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "NEARDUP_HARD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
