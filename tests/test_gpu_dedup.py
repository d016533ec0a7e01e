"""GPU checks of the duplicate-row removal (wp_dedup_rows, wp_dedup_rows_device) against tests/dedup_model.py, exactly:
every output array with its dtype, the offsets and the bytes of the compact form, and the statistics that depend on no
hash — at the chunk edges, with one long row beside short ones, for ids, at degenerate shapes, through the collision
rounds, at the sizes where the sort changes configuration, with bytes behind the data, with bad offsets, across the
states of a handle and end to end with the encoder, the packer and the detokenizer."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import dedup_model as DM
import wordpiece_amd as W

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")
VOCAB = ["[UNK]", "a", "b", "##b", "中", "."]
C = 256           # bytes of a chunk (dedup.h: kDedupChunk)
TILE = 256 * C    # bytes a workgroup of the key and compare kernels covers (dedup.h: kDedupTile)
STAT_KEYS = ("n_rows", "n_unique", "n_empty", "n_elems")


def test_geometry_matches_the_kernels():
    src = open(os.path.join(PKG, "csrc", "dedup.h")).read()
    common = open(os.path.join(PKG, "csrc", "common.h")).read()
    block = int(re.search(r"constexpr int kBlock = (\d+);", common).group(1))
    assert int(re.search(r"constexpr int kDedupChunk = (\d+);", src).group(1)) == C
    assert re.search(r"constexpr int kDedupTile = kBlock \* kDedupChunk;", src) and block * C == TILE
    assert re.search(r"kSiteDedup = 17,", common)
    radix = open(os.path.join(PKG, "csrc", "radix_sort.h")).read()
    assert re.search(r"constexpr size_t kRadixSmallN = size_t\(1\) << 21;", radix)


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
    for key, dtype in (("first", np.int32), ("kept", np.int32), ("counts", np.int64), ("inverse", np.int32), ("row_off", np.int64)):
        assert got[key].dtype == dtype and got[key].tolist() == exp[key], (where, key)
    assert got["data"].dtype == (np.uint8 if eb == 1 else np.int32) and got["data"].tobytes() == exp["data"], (where, "data")


def check(rows, where, eb=1, tensor=False, v=None, hash_bits=0):
    """one call on the rows (bytes each) against the model; -> (the model's answer, the statistics of the call)"""
    import torch
    v = v or handle()
    data, off = DM.join(rows, eb)
    exp = DM.dedup_rows(data, off, eb)
    if tensor:
        got = v.dedup_rows_tensor(to_gpu(data, eb), torch.tensor(off, dtype=torch.int64, device="cuda"), inverse=True, compact=True,
                                  hash_bits=hash_bits)
    else:
        got = v.dedup_rows(np.frombuffer(data, dtype=np.uint8 if eb == 1 else np.int32), off, inverse=True, compact=True, raw=True,
                           hash_bits=hash_bits)
    compare(got, exp, eb, where, tensor)
    st = v.dedup_stats()
    assert {k: st[k] for k in STAT_KEYS} == exp["stats"], where
    if exp["stats"]["n_elems"]:  # (a batch without an element is answered by the host form without a device)
        assert st["n_rounds"] >= 1 and st["n_chunks"] == sum((len(r) + C - 1) // C for r in rows), where
    return exp, st


def pattern(n, salt=0):
    return bytes((7 * i + 13 * (i // C) + salt) % 251 for i in range(n))


def changed(row, at):
    return row[:at] + bytes([row[at] ^ 0x40]) + row[at + 1:]


@pytest.mark.gpu
def test_rows_at_the_chunk_edges():
    lengths = (0, 1, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1)
    rows = []
    for n in lengths:
        base = pattern(n, n)
        rows += [base, base]
        if n >= 1:
            rows += [changed(base, 0), changed(base, n - 1), changed(base, 0)]
        if n > C:
            rows += [changed(base, C - 1), changed(base, C), changed(base, C)]
    # a proper prefix of another row, cut inside a chunk and at a chunk edge
    long = pattern(2 * C + 1, 5)
    rows += [long, long[:C + 17], long[:C], long[:2 * C], long[:C + 17], long[:1]]
    for tensor in (False, True):
        exp, st = check(rows, "chunk edges", tensor=tensor)
        assert st["n_unique"] < len(rows) and st["n_compared"] > 0
        # the same rows at every start offset mod 4
        for lead in (1, 2, 3):
            exp2, _ = check([b"\xee" * lead] + rows, ("start offset", lead), tensor=tensor)
            assert [f - 1 for f in exp2["first"][1:]] == exp["first"]
    # one row per length placed four times, each copy at another offset mod 4: all four are one row
    for n in lengths[1:]:
        base = pattern(n, 3)
        rows, total = [], 0
        for c in range(4):
            if c:
                pad = (c - total) % 4 or 4
                rows.append(b"\xee" * pad)
                total += pad
            assert total % 4 == c
            rows.append(base)
            total += n
        exp, _ = check(rows, ("placed", n), tensor=True)
        assert exp["counts"][0] == 4, n


@pytest.mark.gpu
def test_one_long_row_beside_short_ones():
    n = 3 * TILE + 5
    long = np.random.default_rng(4).integers(0, 256, n, dtype=np.uint8).tobytes()
    other = changed(long, (n // C // 2) * C + 9)  # one byte of the middle chunk
    rng = random.Random(4)
    short = [bytes(rng.randrange(97, 101) for _ in range(3)) for _ in range(1000)]
    rows = short[:300] + [long] + short[300:600] + [other] + short[600:] + [long]
    for tensor in (False, True):
        exp, st = check(rows, "long row", tensor=tensor)
        assert exp["counts"][exp["kept"].index(300)] == 2 and exp["first"][601] == 601 and exp["first"][-1] == 300
        # the second copy is compared with the first over its whole length; a collision apart, nothing else of the long
        # rows is read again, and the short rows add at most their own bytes: work follows the elements
        assert n <= st["n_compared"] <= n + 3 * 1000
        assert st["n_chunks"] == 3 * ((n + C - 1) // C) + 1000 and st["n_rounds"] == 1


@pytest.mark.gpu
def test_ids_rows():
    def ids(*values):
        return np.array(values, dtype=np.int32).tobytes()
    rows = [ids(), ids(5), ids(5, 6), ids(5, 6, 7), ids(), ids(5), ids(5, 6), ids(5, 6, 7),
            ids(5 + (1 << 24)), ids(5 + (2 << 24)), ids(5, 6 + (1 << 24)), ids(5, 6, 7 - (1 << 31)), ids(5 + (1 << 24)),
            ids(6, 5), ids(5, 6), ids(-1), ids(-1, -1), ids(-1)]
    big = np.arange(3 * C // 4 + 1, dtype=np.int32)  # rows of several chunks: equal, and different in the high byte of one id
    rows += [big.tobytes(), big.tobytes(), (big + np.where(np.arange(big.size) == C // 4, 1 << 24, 0).astype(np.int32)).tobytes()]
    for tensor in (False, True):
        exp, st = check(rows, "ids", eb=4, tensor=tensor)
        assert exp["first"][:8] == [0, 1, 2, 3, 0, 1, 2, 3] and exp["first"][12] == 8 and exp["first"][14] == 2
        assert exp["first"][-3:] == [len(rows) - 3, len(rows) - 3, len(rows) - 1]
        assert st["n_elems"] == sum(len(r) for r in rows) // 4  # (the offsets, and n_compared, are in elements)
        assert st["n_compared"] >= big.size


@pytest.mark.gpu
def test_degenerate_shapes():
    import torch
    v = handle()
    for tensor in (False, True):
        check([b"only"], "one row", tensor=tensor)
        check([b"q"], "one byte", tensor=tensor)
        check([pattern(700)], "one row of three chunks", tensor=tensor)
    # all rows empty, device form (the host form answers without a device): with and without a data pointer
    for n in (1, 5, 3000):
        for data in (torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(16, dtype=torch.uint8, device="cuda")):
            got = v.dedup_rows_tensor(data, torch.zeros(n + 1, dtype=torch.int64, device="cuda"), inverse=True, compact=True)
            compare(got, DM.dedup_rows(b"", [0] * (n + 1)), 1, ("all empty", n), True)
            st = v.dedup_stats()
            assert (st["n_rows"], st["n_unique"], st["n_empty"], st["n_elems"], st["n_chunks"], st["n_compared"]) == (n, 1, n, 0, 0, 0)
    got = v.dedup_rows_tensor(torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), compact=True)
    assert got["first"].numel() == 0 and got["kept"].numel() == 0 and got["row_off"].tolist() == [0] and v.dedup_stats()["n_rows"] == 0
    # a hot group, and no group at all
    n = 70_000
    row = b"the same line\n"
    off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * len(row)
    got = v.dedup_rows_tensor(to_gpu(row * n, 1), off, inverse=True, compact=True)
    assert got["first"].dtype == torch.int32 and not got["first"].any() and got["kept"].tolist() == [0] and got["counts"].tolist() == [n]
    assert not got["inverse"].any() and got["data"].cpu().numpy().tobytes() == row and got["row_off"].tolist() == [0, len(row)]
    st = v.dedup_stats()
    assert (st["n_unique"], st["n_compared"], st["n_rounds"]) == (1, (n - 1) * len(row), 1)
    distinct = np.arange(n, dtype=np.int32)
    got = v.dedup_rows_tensor(torch.from_numpy(distinct).cuda(), torch.arange(n + 1, dtype=torch.int64, device="cuda"), inverse=True, compact=True)
    for key in ("first", "kept", "inverse", "data"):
        assert got[key].dtype == torch.int32 and np.array_equal(got[key].cpu().numpy(), distinct), key
    assert got["counts"].dtype == torch.int64 and bool((got["counts"] == 1).all()) and np.array_equal(got["row_off"].cpu().numpy(), np.arange(n + 1))
    assert v.dedup_stats()["n_unique"] == n
    # the documents form and the lines form, through the host call
    docs = ["b", "a", "b", "", "a b", "", "b"]
    assert v.dedup_docs(docs)[0] == ["b", "a", "", "a b"] and v.dedup_docs(docs)[1].tolist() == [3, 1, 2, 1]
    r = v.dedup_rows(b"x\ny\nx\n\nx", compact=True)  # (the last line gets its line feed)
    assert r["kept"].tolist() == [0, 1, 3] and r["counts"].tolist() == [3, 1, 1] and r["data"] == b"x\ny\n\n"


@pytest.mark.gpu
def test_collision_rounds_never_change_a_result():
    rng = random.Random(6)
    rows = [b"%d:" % k + pattern(rng.choice((0, 3, C - 2, C + 5)), k) for k in range(600)]
    rows = rows + [rows[k] for k in range(0, 600, 7)]
    rng.shuffle(rows)
    v = handle()
    results = {}
    for bits in (8, 12, 64, 0):
        for tensor in (False, True):
            exp, st = check(rows, ("hash_bits", bits), hash_bits=bits, tensor=tensor)
            assert st["n_unique"] == 600
            if bits == 8:  # (600 distinct rows on 256 keys: two of them share one)
                assert st["n_rounds"] >= 2 and st["n_collided"] >= 1
            if bits in (64, 0):
                assert st["n_rounds"] == 1 and st["n_collided"] == 0
        data, off = DM.join(rows)
        results[bits] = v.dedup_rows(data, off, inverse=True, compact=True, hash_bits=bits)
    for bits in (12, 64, 0):
        for key in ("first", "kept", "counts", "inverse", "row_off"):
            assert np.array_equal(results[bits][key], results[8][key]), (bits, key)
        assert results[bits]["data"] == results[8]["data"]
    # leftovers of round 0 that hold duplicates of each other: 300 distinct rows, each three times, on 256 keys
    rows = [b"r%03d" % k + b"z" * (k % 5) for k in range(300)] * 3
    for tensor in (False, True):
        exp, st = check(rows, "duplicates among the leftovers", hash_bits=8, tensor=tensor)
        assert st["n_rounds"] >= 2 and st["n_collided"] >= 3 and exp["counts"] == [3] * 300


def _check_big(n, seed):
    """n rows of 0..2 bytes over two byte values, through the tensor form, against numpy.unique over the rows as numbers"""
    import torch
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 3, n).astype(np.int64)
    off = np.concatenate(([0], np.cumsum(lens)))
    data = rng.integers(120, 122, int(off[-1]), dtype=np.uint8)
    b0 = np.where(lens >= 1, data[np.minimum(off[:-1], data.size - 1)], 0).astype(np.int64)
    b1 = np.where(lens >= 2, data[np.minimum(off[:-1] + 1, data.size - 1)], 0).astype(np.int64)
    exp = DM.dedup_fixed((lens * 65536 + b0 * 256 + b1).reshape(-1, 1))
    v = handle()
    got = v.dedup_rows_tensor(torch.from_numpy(data).cuda(), torch.from_numpy(off).cuda(), inverse=True, compact=True, copy=False)
    for key in ("first", "kept", "counts", "inverse"):
        assert got[key].cpu().numpy().dtype == exp[key].dtype and np.array_equal(got[key].cpu().numpy(), exp[key]), (n, key)
    kept = exp["kept"].astype(np.int64)
    assert np.array_equal(got["row_off"].cpu().numpy(), np.concatenate(([0], np.cumsum(lens[kept]))))
    assert got["data"].cpu().numpy().tobytes() == b"".join(data[off[k]:off[k + 1]].tobytes() for k in kept)
    st = v.dedup_stats()
    assert (st["n_rows"], st["n_unique"], st["n_empty"], st["n_elems"]) == (n, kept.size, int((lens == 0).sum()), int(off[-1]))
    assert kept.size == 7 and st["n_chunks"] == n - st["n_empty"]


@pytest.mark.gpu
def test_row_counts_around_the_small_sort():
    _check_big(2 ** 21 - 1, 1)
    _check_big(2 ** 21 + 1, 2)


@pytest.mark.gpu
def test_bytes_behind_the_data_are_not_read():
    import torch
    v = handle()
    rows = [pattern(C + 3, 1), b"ab", pattern(C + 3, 1), b"ab", pattern(5, 2), b"abc"]
    data, off = DM.join(rows)
    assert len(data) % 4 != 0
    exp = DM.dedup_rows(data, off)
    off_t = torch.tensor(off, dtype=torch.int64, device="cuda")
    for fill in (0x00, 0xff, 0x61):
        big = torch.full((len(data) + 4096,), fill, dtype=torch.uint8, device="cuda")
        big[:len(data)] = to_gpu(data, 1)
        view = big[:(len(data) + 259) // 4 * 4]  # a prefix view that is aligned and whole words long: it is passed as it is
        assert view.data_ptr() == big.data_ptr() and view.numel() > len(data)
        compare(v.dedup_rows_tensor(view, off_t, inverse=True, compact=True), exp, 1, ("trailing", fill), True)
        assert v.dedup_stats()["n_elems"] == len(data)
    # a text whose last row ends on the last byte of its tensor, at every length mod 4
    for extra in range(4):
        rows2 = rows + [b"z" * extra, b"abc"]
        data2, off2 = DM.join(rows2)
        compare(v.dedup_rows_tensor(to_gpu(data2, 1), torch.tensor(off2, dtype=torch.int64, device="cuda"), inverse=True, compact=True),
                DM.dedup_rows(data2, off2), 1, ("last byte", extra), True)
    # ids behind the last row
    ids = np.array([3, 4, 3, 4, 9, 9, 9], dtype=np.int32)
    got = v.dedup_rows_tensor(torch.from_numpy(ids).cuda(), torch.tensor([0, 2, 4], dtype=torch.int64, device="cuda"), compact=True)
    assert got["first"].tolist() == [0, 0] and got["data"].tolist() == [3, 4] and v.dedup_stats()["n_elems"] == 4


@pytest.mark.gpu
def test_bad_offsets_in_the_device_form():
    import torch
    v = W.Vocab(VOCAB)
    data = to_gpu(b"abcdefghijklmnop", 1)
    good = [0, 2, 4, 6, 8, 10, 12]
    for bad_row, off in ((0, [0, -1, 4, 6, 8, 10, 12]), (0, [1, 2, 4, 6, 8, 10, 12]), (3, [0, 2, 4, 7, 6, 10, 12]), (5, [0, 2, 4, 6, 8, 10, 9]),
                         (1, [0, 5, 4, 3, 8, 10, 12]), (2, [0, 2, 2 ** 40, 6, 8, 10, 12])):
        with pytest.raises(W.WordPieceError, match=r"row_off must .* row %d$" % bad_row):
            v.dedup_rows_tensor(data, torch.tensor(off, dtype=torch.int64, device="cuda"))
        got = v.dedup_rows_tensor(data, torch.tensor(good, dtype=torch.int64, device="cuda"))  # the handle is usable afterwards
        assert got["first"].tolist() == list(range(6)) and v.dedup_stats()["n_unique"] == 6
    with pytest.raises(W.WordPieceError, match="UINT32_MAX"):
        v.dedup_rows_tensor(data, torch.tensor([0, 2, 2 ** 33], dtype=torch.int64, device="cuda"))
    assert v.encode("ab a").tolist() == [1, 3, 1]


@pytest.mark.gpu
def test_handle_state():
    import torch
    v = W.Vocab(VOCAB)
    assert v.dedup_stats()["n_rows"] == -1
    small = [b"ab", b"a", b"ab"]
    large = [pattern(k % 700, k % 50) for k in range(5000)]
    check(small, "first call", v=v)
    text = ("b a b . 中 ab a b " * 40).encode("utf8")
    ids = v.encode(text)
    assert len(ids) == 9 * 40 and v.dedup_stats()["n_rows"] == -1  # (an encode since: as every layer's statistics)
    check(large, "grown", v=v, tensor=True)
    words = v.count_words(text)
    assert words["counts"].sum() == 8 * 40
    check(small + [b""], "shrunk, behind a count call", v=v, tensor=True)
    assert v.encode(text).tolist() == ids.tolist()
    # views live until the handle's next call, whatever other handles do
    data, off = DM.join(large)
    d, o = to_gpu(data, 1), torch.tensor(off, dtype=torch.int64, device="cuda")
    views = v.dedup_rows_tensor(d, o, inverse=True, compact=True, copy=False)
    kept = {k: x.clone() for k, x in views.items()}
    other = W.Vocab(["x", "b a"])
    other.dedup_rows_tensor(d[:o[40]], o[:41], inverse=True, compact=True)
    other.encode(text)
    assert all(torch.equal(views[k], kept[k]) for k in views)
    copies = v.dedup_rows_tensor(d, o, inverse=True, compact=True)
    assert all(torch.equal(copies[k], kept[k]) for k in kept)
    for rows, trim in ((small, False), (large, False), ([b"q"], True), (large[:900], False)):
        if trim:
            v.trim()
        check(rows, ("sizes", len(rows), trim), v=v, tensor=trim)


@pytest.mark.gpu
def test_end_to_end_with_the_encoder_the_packer_and_the_detokenizer():
    import torch
    import normalize_model as NM
    import oracle_lib as O
    vocab = ["[UNK]", "[CLS]", "[SEP]", "hello", "world", ",", "cafe", "##s", "a", "b", "the", "##x"]
    docs = ["Hello, World", "hello,  world", "cafés", "the a b", "HELLO , WORLD", "CAFES", "the  a b", "", "world hello", "The A B",
            " ", "a b " * 100, "A  B " * 100, "world hello"]
    v = W.Vocab(vocab, normalize=W.WP_NORM_BERT_UNCASED)
    oracle = O.Vocab(vocab)
    want_ids = [np.asarray(oracle.encode(NM.normalize(d.encode("utf8"), W.WP_NORM_BERT_UNCASED)[0]), dtype=np.int32) for d in docs]
    exp = DM.dedup_rows(*DM.join([w.tobytes() for w in want_ids], 4), elem_bytes=4)
    text, off = W.join_docs(docs)
    t = torch.zeros((len(text) + 19) // 16 * 16, dtype=torch.uint8, device="cuda")
    t[:len(text)] = to_gpu(text, 1)
    ids, splits = v.encode_rows_tensor(t[:len(text)], torch.from_numpy(off).cuda())
    got = v.dedup_rows_tensor(ids, splits, inverse=True, compact=True)
    compare(got, exp, 4, "ids of the rows call", True)
    # lines that differ only in case, accents or blank runs are one document to the model
    assert exp["first"][:7] == [0, 0, 2, 3, 0, 2, 3] and exp["first"][9] == 3 and exp["first"][10] == 7 and exp["first"][12] == 11
    assert len(exp["kept"]) == 6
    # the text itself keeps them apart
    raw = v.dedup_rows_tensor(t[:len(text)], torch.from_numpy(off).cuda())
    assert raw["kept"].numel() == len(set(docs)) == 13
    # the compact form is what the packer takes; its rows, detokenized, are the kept documents
    packed = v.pack_sequences_tensor(got["data"], got["row_off"], max_len=512)
    texts = v.detokenize(got["data"].cpu().numpy(), row_splits=got["row_off"].cpu().numpy())
    assert texts == ["hello, world", "cafes", "the a b", "", "world hello", ("a b " * 100).strip()]
    flat = np.frombuffer(exp["data"], dtype=np.int32)  # (210 ids: next fit puts the six documents into one row)
    assert packed["lengths"].tolist() == [flat.size] and packed["input_ids"][0, :flat.size].tolist() == flat.tolist()
    assert packed["segment_ids"][0, :flat.size].unique().tolist() == [1, 2, 3, 4, 5]  # (the empty document takes no cell)
    # the table of a count call is distinct already: every word is kept
    table = v.count_words_tensor(t[:len(text)], terminator="\n")
    kept = v.dedup_rows_tensor(table["words"], table["word_off"])
    n = table["counts"].numel()
    assert n > 5 and kept["kept"].tolist() == list(range(n)) and bool((kept["counts"] == 1).all())


@pytest.mark.gpu
@pytest.mark.parametrize("lib_name,guard", [("libwordpiece_amd_dbg.so", "0"), ("libwordpiece_amd.so", "1")])
def test_hardened_runs(tmp_path, lib_name, guard):
    """(a fresh child: once on the bounds-checking build, once with WP_ARENA_GUARD=1) the chunk-edge and the collision
    cases: no store or gather outside an array (kSiteDedup, kSiteGroup), no guard zone of the call's arenas overwritten"""
    lib = os.path.join(PKG, lib_name)
    assert os.path.exists(lib), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "dedup_hard_run.py"
    script.write_text('''
import sys
import torch  # (before the library, as tests/conftest.py: the HIP runtime loaded first serves the process)
sys.path.insert(0, %r); sys.path.insert(0, %r)
import wordpiece_amd as W
import test_gpu_dedup as T
v = T.handle()
v.encode("ab a")
assert v.stats()["reserved0"] == %d, "not the build this run is about"
T.test_rows_at_the_chunk_edges()
T.test_collision_rounds_never_change_a_result()
T.test_ids_rows()
print("DEDUP_HARD_OK")
''' % (os.path.dirname(PKG), HERE, 1 if "dbg" in lib_name else 0))
    env = dict(os.environ, WP_LIB=lib, WP_ARENA_GUARD=guard)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "DEDUP_HARD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
