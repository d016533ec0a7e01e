"""GPU checks of the n-gram overlap search (wp_overlap_rows, wp_overlap_rows_device) against tests/overlap_model.py,
exactly: every output array with its dtype, the compact form and the statistics the contract fixes — at every window
shape, at the tile and halo edges of the window kernel, with one long row beside short ones, on repeated reference
windows, under key collisions, with bytes behind the data, with bad offsets, across the states of a handle and end to
end with the encoder and the packer."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import overlap_cases as K
import overlap_model as M
import wordpiece_amd as W

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")
VOCAB = ["[UNK]", "a", "b", "##b", "中", "."]
T = K.tile()  # window positions per workgroup of the key kernel (overlap.h: kOvlTile)
ARG = 6


def test_geometry_matches_the_kernels():
    src = open(os.path.join(PKG, "csrc", "overlap.h")).read()
    common = open(os.path.join(PKG, "csrc", "common.h")).read()
    block = int(re.search(r"constexpr int kBlock = (\d+);", common).group(1))
    items = int(re.search(r"constexpr int kOvlItems = (\d+);", src).group(1))
    assert re.search(r"constexpr int kOvlSpan = kBlock \* kOvlItems;", src) and re.search(r"constexpr int kOvlMaxNgram = 64;", src)
    assert T + 64 <= block * items  # the halo of the last position of a tile lies inside what the workgroup reads
    assert re.search(r"kSiteOverlap = 19,", common) and re.search(r"kSiteNearDup = 18,", common)


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


def off_gpu(off):
    import torch
    return torch.tensor(off, dtype=torch.int64, device="cuda")


def compare(got, exp, eb, where, tensor):
    """every array of one call against the model's, dtype included"""
    if tensor:
        got = {k: x.cpu().numpy() for k, x in got.items()}
    for key, dtype in (("hits", np.int64), ("first_hit", np.int64), ("first_ref", np.int32), ("covered", np.int64), ("mask", np.uint8),
                       ("ref_hits", np.int64), ("kept", np.int32), ("row_off", np.int64)):
        assert got[key].dtype == dtype, (where, key, got[key].dtype)
        if not np.array_equal(got[key], np.asarray(exp[key], dtype=dtype)):
            bad = np.flatnonzero(got[key] != np.asarray(exp[key], dtype=dtype)) if len(got[key]) == len(exp[key]) else []
            raise AssertionError((where, key, len(got[key]), len(exp[key]), [(int(i), int(got[key][i]), int(exp[key][i])) for i in bad[:5]]))
    assert got["data"].dtype == (np.uint8 if eb == 1 else np.int32) and got["data"].tobytes() == exp["data"], (where, "data")


def check(rows, refs, where, eb=1, forms=(False, True), v=None, exp=None, **spec):
    """the corpus rows and the reference rows (bytes each) through the host form and the tensor form against the model;
    -> (the model's answer, the statistics of the last call)"""
    v = v or handle()
    data, off = M.join(rows, eb)
    rdata, roff = M.join(refs, eb)
    model_spec = {k: x for k, x in spec.items() if k != "hash_bits"}
    exp = exp or M.overlap_rows(data, off, rdata, roff, elem_bytes=eb, **model_spec)
    st = None
    for tensor in forms:
        if tensor:
            got = v.overlap_rows_tensor(to_gpu(data, eb), off_gpu(off), to_gpu(rdata, eb), off_gpu(roff), mask=True, ref=True, compact=True, **spec)
        else:
            dt = np.uint8 if eb == 1 else np.int32
            got = v.overlap_rows(np.frombuffer(data, dtype=dt), off, np.frombuffer(rdata, dtype=dt), roff, mask=True, ref=True, compact=True,
                                 raw=True, **spec)
        compare(got, exp, eb, (where, "tensor" if tensor else "host"), tensor)
        st = v.overlap_stats()
        assert {k: st[k] for k in exp["stats"]} == exp["stats"], (where, st, exp["stats"])
        assert st["n_hits"] <= st["n_candidates"] <= st["n_windows"], (where, st)
    return exp, st


def elems(values, eb):
    """elements of a small alphabet as a row: bytes, or ids"""
    a = np.asarray(values)
    assert a.size == 0 or (eb == 4 or a.max() < 256)
    return bytes(a.astype(np.uint8)) if eb == 1 else (a + 1000).astype(np.int32).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("eb", [1, 4])
def test_window_shapes_short_rows_and_empty_rows(eb):
    rng = np.random.default_rng(10 + eb)
    for k in (1, 2, 13, 63, 64):
        src = rng.integers(0, 4, 400)
        ref_rows = [elems(src[:k + 40], eb), b"", elems(src[100:100 + k], eb), elems(src[150:150 + max(k - 1, 0)], eb)]
        rows = [b"", b"", elems(src[5:5 + k - 1], eb), elems(src[5:5 + k], eb), elems(src[5:5 + k + 1], eb), b"", b"", b"",
                elems(rng.integers(0, 4, k + 30), eb), elems(src[90:120 + k], eb), elems(src[100:100 + k], eb), b"", b""]
        exp, st = check(rows, ref_rows, ("shapes", k), eb, ngram=k)
        assert exp["hits"][2] == 0 and exp["hits"][3] == 1 and exp["hits"][4] == 2 and exp["hits"][10] == 1, k
        assert st["n_windows"] == sum(max(len(r) // eb - k + 1, 0) for r in rows)
        check(rows, [], ("no reference row", k), eb, ngram=k, forms=(True,))
        check(rows, [b"", elems(src[:k - 1], eb)], ("no reference window", k), eb, ngram=k, forms=(True,))
        check([b"", elems(src[:k - 1], eb), b""], ref_rows, ("no corpus window", k), eb, ngram=k, forms=(True,))


@pytest.mark.gpu
@pytest.mark.parametrize("eb,k", [(4, 1), (4, 2), (4, 13), (4, 63), (4, 64), (1, 13), (1, 64), (1, 2)])
def test_tile_and_halo_edges(eb, k):
    rows, refs, eb, facts = K.tile_edge_case(T, k, eb)
    exp, st = check(rows, refs, ("tile edge", eb, k), eb, ngram=k)
    assert exp["first_hit"][0] <= facts["planted"][0] and exp["hits"][0] >= len(facts["planted"])
    if k >= 2:
        for shift in (-1, 0, 1):
            brows, brefs, _, bfacts = K.boundary_case(T, k, eb, T + shift)
            bexp, _ = check(brows, brefs, ("boundary", eb, k, shift), eb, ngram=k)
            assert k < 4 and eb == 1 or bexp["hits"] == [0, 0]  # (the bytes across the boundary are a reference window: test_overlap_model.py)


@pytest.mark.gpu
@pytest.mark.parametrize("eb", [1, 4])
def test_one_window_per_row_over_a_whole_tile(eb):
    rows, refs, eb, facts = K.unit_rows_case(T, 5, eb)
    exp, st = check(rows, refs, ("unit rows", eb), eb, ngram=5)
    assert [i for i, h in enumerate(exp["hits"]) if h] == facts["hit_rows"] and st["n_windows"] == T
    check(rows, refs, ("unit rows, kept", eb), eb, ngram=5, max_hits=1, forms=(True,))


_long = {}


def long_case():
    """the long-row case and the model's answer to it, computed once"""
    if not _long:
        rows, refs, eb, facts = K.long_row_case()
        data, off = M.join(rows, eb)
        rdata, roff = M.join(refs, eb)
        _long.update(rows=rows, refs=refs, facts=facts, exp=M.overlap_rows(data, off, rdata, roff, elem_bytes=eb, ngram=13))
    return _long


@pytest.mark.gpu
def test_one_long_row_beside_short_ones():
    c = long_case()
    exp, st = check(c["rows"], c["refs"], "long row", 4, exp=c["exp"], ngram=13)
    long = c["facts"]["long"]
    assert exp["hits"][long] == c["facts"]["hits"] == st["n_hits"] and exp["covered"][long] == c["facts"]["covered"] < 13 * st["n_hits"]
    assert 0.24 < st["n_hits"] / st["n_windows"] < 0.26 and st["n_hit_rows"] == 1 and exp["kept"] == [i for i in range(51) if i != long]


@pytest.mark.gpu
@pytest.mark.parametrize("eb", [1, 4])
def test_reference_multiplicity(eb):
    rng = np.random.default_rng(20 + eb)
    k = 7
    leak = elems(rng.integers(0, 50, 30), eb)      # a reference row that leaks twice into one corpus row and once into another
    shared = elems(rng.integers(50, 100, k), eb)   # the same window in reference rows 7 and 3
    filler = [elems(rng.integers(100, 150, 12), eb) for _ in range(8)]
    refs = [filler[0], elems(np.zeros(5000, dtype=np.int64) + 151, eb), leak, filler[1] + shared, filler[2], filler[3], filler[4],
            shared + filler[5], filler[6]]
    w = k * eb
    rows = [filler[7] + leak[:w] + filler[7] + leak[3 * eb:3 * eb + w], elems(rng.integers(160, 200, 20), eb), filler[7] + leak[:w] + shared,
            elems(np.zeros(k + 3, dtype=np.int64) + 151, eb), b"", shared]
    exp, st = check(rows, refs, ("multiplicity", eb), eb, ngram=k)
    assert exp["first_ref"] == [2, -1, 2, 1, -1, 3] and exp["hits"] == [2, 0, 2, 4, 0, 1]
    assert exp["ref_hits"] == [0, 5000 - k + 1, 2, 1, 0, 0, 0, 1, 0]  # (windows are counted once each, however often they leak)
    assert st["n_ref_distinct"] == st["n_ref_windows"] - (5000 - k) - 1


@pytest.mark.gpu
@pytest.mark.parametrize("eb", [1, 4])
def test_key_collisions_change_nothing(eb):
    rng = np.random.default_rng(30 + eb)
    k = 6
    refs = [elems(rng.integers(0, 90, 40), eb) for _ in range(20)] + [elems(rng.integers(0, 90, 40), eb)] * 2  # 700 windows and a repeated row
    rows = [refs[3][5 * eb:25 * eb], elems(rng.integers(0, 90, 300), eb), refs[7] + refs[8], b"", elems(rng.integers(100, 190, 400), eb),
            refs[21][2 * eb:(2 + k) * eb]]
    wide, st_wide = check(rows, refs, ("64 bits", eb), eb, ngram=k)
    narrow, st = check(rows, refs, ("8 bits", eb), eb, exp=wide, ngram=k, hash_bits=8)
    assert st["n_ref_distinct"] >= 600 and st["n_collided"] > 0  # (more than 256 distinct windows on 256 keys)
    assert st_wide["n_collided"] == 0 and st_wide["n_candidates"] == st_wide["n_hits"]
    # 700 non-hitting corpus windows on 256 keys that hold 600 entries: candidates that are no hits
    assert st["n_candidates"] > st["n_hits"] > 0
    for bits in (9, 16, 33, 63):
        check(rows, refs, (bits, eb), eb, exp=wide, ngram=k, hash_bits=bits, forms=(True,))


@pytest.mark.gpu
@pytest.mark.parametrize("eb", [1, 4])
def test_dirty_bytes_behind_the_data_and_every_byte_phase(eb):
    import torch
    rng = np.random.default_rng(40 + eb)
    k = 5
    v = handle()
    for phase in range(4):
        refs = [elems(rng.integers(0, 3, 1 + phase), eb), elems(rng.integers(0, 3, 22), eb), elems(rng.integers(0, 3, 9), eb)]
        rows = [elems(rng.integers(0, 3, phase), eb), elems(rng.integers(0, 3, 17), eb), elems(rng.integers(0, 3, 6), eb),
                elems(rng.integers(0, 3, 11), eb) + refs[1][2 * eb:14 * eb] + elems(rng.integers(0, 3, 7), eb)]  # (a planted span: 8 hits at least)
        for batch in (rows, refs):  # (a whole number of words, so that the tensors are read where they lie, with 0xff behind them)
            n = sum(len(r) for r in batch)
            batch.append(elems(rng.integers(0, 3, (-n // eb) % 4 + 4), eb))
        data, off = M.join(rows, eb)
        rdata, roff = M.join(refs, eb)
        exp = M.overlap_rows(data, off, rdata, roff, elem_bytes=eb, ngram=k)
        big, rbig = (torch.full((len(d) // eb + 4096,), 0xff if eb == 1 else -1, dtype=torch.uint8 if eb == 1 else torch.int32, device="cuda")
                     for d in (data, rdata))
        big[:len(data) // eb] = to_gpu(data, eb)
        rbig[:len(rdata) // eb] = to_gpu(rdata, eb)
        got = v.overlap_rows_tensor(big[:len(data) // eb], off_gpu(off), rbig[:len(rdata) // eb], off_gpu(roff), ngram=k, mask=True, ref=True,
                                    compact=True)
        compare(got, exp, eb, ("dirty", eb, phase), True)
        assert sum(exp["hits"]) > 0 and {k_: v.overlap_stats()[k_] for k_ in exp["stats"]} == exp["stats"]


@pytest.mark.gpu
def test_compact_form_and_the_packer():
    import torch
    rng = np.random.default_rng(50)
    k = 4
    ref = elems(rng.integers(0, 200, 60), 4)
    clean = [elems(rng.integers(200, 400, n), 4) for n in (9, 0, 25, 3)]
    rows = [clean[0], ref[:5 * 4] + clean[2], clean[1], ref[8 * 4:15 * 4], clean[2], clean[3], ref[20 * 4:24 * 4]]
    top = None
    for max_hits in (0, 1, 2, 1000):
        exp, st = check(rows, [ref], ("max_hits", max_hits), 4, ngram=k, max_hits=max_hits)
        top = exp
    assert top["hits"] == [0, 2, 0, 4, 0, 0, 1] and top["kept"] == list(range(7))
    exp, _ = check([rows[1], rows[3], rows[6]], [ref], "all rows dropped", 4, ngram=k)
    assert exp["kept"] == [] and exp["row_off"] == [0] and exp["data"] == b""
    v = handle()
    data, off = M.join(rows, 4)
    got = v.overlap_rows_tensor(to_gpu(data, 4), off_gpu(off), to_gpu(ref, 4), off_gpu([0, 60]), ngram=k, compact=True)
    assert got["kept"].tolist() == [0, 2, 4, 5] and sorted(got) == ["covered", "data", "first_hit", "first_ref", "hits", "kept", "row_off"]
    packed = v.pack_sequences_tensor(got["data"], got["row_off"], max_len=64)
    assert int(packed["lengths"].sum()) == 9 + 25 + 3 and got["data"].dtype == torch.int32


@pytest.mark.gpu
def test_bad_offsets_in_the_device_form_name_the_batch_and_the_first_bad_row():
    import torch
    v = W.Vocab(VOCAB)
    data = to_gpu(b"abcdefgh" * 8, 1)
    good = off_gpu([0, 4, 8, 20])
    for off, row in (([1, 2, 3], 0), ([0, 3, 2, 8], 1), ([0, 2, 4, 3], 2), ([0, 4, 2, 1], 1), ([-1, 2], 0), ([0, -1], 0), ([0, 2 ** 40, 3], 1)):
        for name, args in (("row_off", (data, off_gpu(off), data, good)), ("ref_off", (data, good, data, off_gpu(off)))):
            other = "ref_off" if name == "row_off" else "row_off"
            with pytest.raises(W.WordPieceError) as e:
                v.overlap_rows_tensor(*args, ngram=2)
            assert name in str(e.value) and other not in str(e.value) and str(e.value).endswith("row %d" % row), (off, name, str(e.value))
    r = v.overlap_rows_tensor(data, good, data, off_gpu([0, 2]), ngram=2)  # the handle works on
    assert r["hits"].tolist() == [1, 0, 2] and torch.equal(r["first_hit"].cpu(), torch.tensor([0, -1, 0]))


@pytest.mark.gpu
def test_handle_states():
    import torch
    import dedup_model as DM
    v = W.Vocab(VOCAB)
    assert v.overlap_stats()["n_rows"] == -1
    rng = np.random.default_rng(60)
    refs = [elems(rng.integers(0, 3, 30), 1) for _ in range(5)]
    small = [b"abcabc", b"", refs[2][3:20]]
    large = [elems(rng.integers(0, 3, int(n)), 1) for n in rng.integers(0, 60, 3000)]
    check(small, refs, "first call", v=v, ngram=6)
    text = ("b a b . 中 ab a b " * 40).encode("utf8")
    ids = v.encode(text)
    assert len(ids) == 9 * 40 and v.overlap_stats()["n_rows"] == -1  # (an encode since: as every layer's statistics)
    check(large, refs, "grown", v=v, ngram=6, forms=(True,))
    assert v.dedup_stats()["n_rows"] == -1
    d = v.dedup_rows(*DM.join(large), compact=True)
    assert d["kept"].tolist() == DM.dedup_rows(*DM.join(large))["kept"] and v.overlap_stats()["n_rows"] == 3000  # (each layer keeps its own)
    v.neardup_rows(*DM.join(large[:50]))
    check(small + [b""], refs[:2], "shrunk, behind a dedup and a neardup call", v=v, ngram=6, forms=(True,))
    assert v.encode(text).tolist() == ids.tolist() and v.overlap_stats()["n_rows"] == -1
    # views live until the handle's next call, whatever other handles do
    data, off = M.join(large)
    rdata, roff = M.join(refs)
    dt, ot, rt, rot = to_gpu(data, 1), off_gpu(off), to_gpu(rdata, 1), off_gpu(roff)
    views = v.overlap_rows_tensor(dt, ot, rt, rot, ngram=6, mask=True, ref=True, compact=True, copy=False)
    kept = {k: x.clone() for k, x in views.items()}
    other = W.Vocab(["x", "b a"])
    other.overlap_rows_tensor(dt[:ot[40]], ot[:41], rt, rot, ngram=3, mask=True, ref=True, compact=True)
    other.encode(text)
    assert all(torch.equal(views[k], kept[k]) for k in views)
    copies = v.overlap_rows_tensor(dt, ot, rt, rot, ngram=6, mask=True, ref=True, compact=True)
    assert all(torch.equal(copies[k], kept[k]) for k in kept)
    for rows, trim in ((small, False), (large[:700], False), ([b"q"], True), (large[:90], False)):
        if trim:
            v.trim()
        check(rows, refs, ("sizes", len(rows), trim), v=v, ngram=6, forms=(trim,))


@pytest.mark.gpu
def test_stage_timing_names_the_table_on_its_own():
    v = W.Vocab(VOCAB)
    v.set_option(W.WP_OPT_STAGE_TIMING, 1)
    c = long_case()
    check(c["rows"], c["refs"], "timed", 4, v=v, exp=c["exp"], ngram=13, forms=(True,))
    s = v.stats()
    assert s["ms_sa"] > 0 and s["ms_scan"] > 0 and s["ms_walk"] > 0 and s["ms_decode"] > 0 and s["ms_normalize"] == 0
    assert abs(s["ms_total"] - (s["ms_decode"] + s["ms_sa"] + s["ms_scan"] + s["ms_walk"])) < 1e-3


@pytest.mark.gpu
def test_end_to_end_with_the_encoder_and_the_packer():
    import torch
    vocab = ["[UNK]", "[CLS]", "[SEP]", "hello", "world", ",", "cafe", "##s", "a", "b", "the", "##x", "of", "and", "is", "in"]
    words = ["the", "world", "of", "cafes", "is", "in", "and", "hello", "a", "cafe", "b", ","]
    rng = np.random.default_rng(70)

    def line(n):
        return " ".join(words[i] for i in rng.integers(0, len(words), n))
    evals = [line(20) for _ in range(20)]
    docs = [line(int(n)) for n in rng.integers(5, 40, 200)]
    dirty = [11, 50, 51, 120, 199]
    for i, d in enumerate(dirty):  # an eval line inside, with changed case, accents and spacing
        docs[d] = (line(3) + " " + evals[3 * i] + " " + line(4)).upper().replace("CAFE", "CAFÉ").replace(" ", "  ")
    v = W.Vocab(vocab, normalize=W.WP_NORM_BERT_UNCASED)

    def encoded(lines):
        text, off = W.join_docs(lines)
        t = torch.zeros((len(text) + 19) // 16 * 16, dtype=torch.uint8, device="cuda")
        t[:len(text)] = to_gpu(text, 1)
        return v.encode_rows_tensor(t[:len(text)], torch.from_numpy(off).cuda()), (t[:len(text)], torch.from_numpy(off).cuda())
    (ids, splits), (text, off) = encoded(docs)
    (rids, rsplits), (rtext, roff) = encoded(evals)
    got = v.overlap_rows_tensor(ids, splits, rids, rsplits, ngram=8, mask=True, ref=True, compact=True)
    exp = M.overlap_rows(ids.cpu().numpy().tobytes(), splits.tolist(), rids.cpu().numpy().tobytes(), rsplits.tolist(), elem_bytes=4, ngram=8)
    compare(got, exp, 4, "ids of the rows call", True)
    assert [i for i, h in enumerate(exp["hits"]) if h] == dirty and exp["first_ref"][11] == 0 and exp["first_ref"][199] == 12
    assert [j for j, h in enumerate(exp["ref_hits"]) if h] == [0, 3, 6, 9, 12] and exp["kept"] == [i for i in range(200) if i not in dirty]
    packed = v.pack_sequences_tensor(got["data"], got["row_off"], max_len=128)
    assert int(packed["lengths"].sum()) == int(got["row_off"][-1]) == len(ids) - sum(int(splits[d + 1] - splits[d]) for d in dirty)
    # the raw bytes do not see through case, accents and spacing
    raw = v.overlap_rows_tensor(text, off, rtext, roff, ngram=8)
    assert not all(int(raw["hits"][d]) for d in dirty)
    # documents that hold an eval line as it stands are what overlap_docs drops
    plain = list(docs)
    for i, d in enumerate(dirty):
        plain[d] = line(2) + " " + evals[3 * i] + " " + line(2)
    clean, hits = v.overlap_docs(plain, evals, ngram=40)
    assert len(clean) == 195 and clean == [plain[i] for i in range(200) if i not in dirty] and [i for i, h in enumerate(hits) if h] == dirty


@pytest.mark.gpu
def test_random_parity():
    rng = np.random.default_rng(80)
    v = handle()
    for it in range(200):
        eb = 1 if it % 2 else 4
        k = int(rng.integers(1, 9))
        rows = [elems(rng.integers(0, 3, int(n)), eb) for n in rng.integers(0, 41, int(rng.integers(1, 12)))]
        refs = [elems(rng.integers(0, 3, int(n)), eb) for n in rng.integers(0, 41, int(rng.integers(0, 11)))]
        check(rows, refs, ("random", it, eb, k), eb, v=v, ngram=k, max_hits=int(rng.integers(0, 4)), hash_bits=(0, 8, 12)[it % 3])


@pytest.mark.gpu
@pytest.mark.parametrize("lib_name,guard", [("libwordpiece_amd_dbg.so", "0"), ("libwordpiece_amd.so", "1")])
def test_hardened_runs(tmp_path, lib_name, guard):
    """(a fresh child: once on the bounds-checking build, once with WP_ARENA_GUARD=1) the tile-edge, the collision and the
    long-row cases: no gather or store outside an array (kSiteOverlap, kSiteGroup), no guard zone of the call's
    arenas overwritten"""
    lib = os.path.join(PKG, lib_name)
    assert os.path.exists(lib), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "overlap_hard_run.py"
    script.write_text('''
import sys
import torch  # (before the library, as tests/conftest.py: the HIP runtime loaded first serves the process)
sys.path.insert(0, %r); sys.path.insert(0, %r)
import wordpiece_amd as W
import test_gpu_overlap as T
v = T.handle()
v.encode("ab a")
assert v.stats()["reserved0"] == %d, "not the build this run is about"
for eb, k in ((4, 1), (4, 13), (4, 64), (1, 13), (1, 64)):
    T.test_tile_and_halo_edges(eb, k)
T.test_one_window_per_row_over_a_whole_tile(1)
T.test_key_collisions_change_nothing(4)
T.test_compact_form_and_the_packer()
T.test_one_long_row_beside_short_ones()
print("OVERLAP_HARD_OK")
''' % (os.path.dirname(PKG), HERE, 1 if "dbg" in lib_name else 0))
    env = dict(os.environ, WP_LIB=lib, WP_ARENA_GUARD=guard)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "OVERLAP_HARD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
