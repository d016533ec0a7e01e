"""GPU checks of the repeated-span search (wp_repeat_rows, wp_repeat_rows_device) against tests/repeat_model.py, exactly:
every output array with its dtype, the cut, the compact form and the statistics the contract fixes — at every window
shape, at the tile and halo edges of the window, flag, cover and cut kernels, with one long row beside short ones, on
windows of every multiplicity, under key collisions, with bytes behind the data, with bad offsets, across the states of
a handle and end to end with the encoder, the exact dedup and the packer."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import repeat_cases as K
import repeat_model as M
import wordpiece_amd as W

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")
VOCAB = ["[UNK]", "a", "b", "##b", "中", "."]
G = K.tiles()
T = G["T"]  # window positions per workgroup of the key kernel (overlap.h: kOvlTile)
ARG = 6
ARRAYS = (("repeats", np.int64), ("first_repeat", np.int64), ("first_src_row", np.int32), ("first_src_pos", np.int64), ("covered", np.int64),
          ("mask", np.uint8), ("src", np.int64), ("kept", np.int32), ("row_off", np.int64), ("cut_off", np.int64))
elems = K.elems


def test_geometry_matches_the_kernels():
    src = open(os.path.join(PKG, "csrc", "repeat.h")).read()
    common = open(os.path.join(PKG, "csrc", "common.h")).read()
    block = int(re.search(r"constexpr int kBlock = (\d+);", common).group(1))
    assert G["tile"] == int(re.search(r"constexpr int kRepTile = (\d+);", src).group(1)) and G["tile"] % block == 0
    assert re.search(r"constexpr int kRepHalo = kOvlMaxNgram;", src) and G["halo"] == 64  # k - 1 elements in front of a tile lie inside the halo
    assert G["cut"] == block * 4 * int(re.search(r"constexpr int kRepCutWords = (\d+);", src).group(1))
    assert re.search(r'#include "overlap.h"', src) and "ovl_keys_kernel" not in src.split("namespace wp")[1]  # the shared kernels are included, not copied
    assert re.search(r"kSiteRepeat = 20,", common) and re.search(r"kSiteOverlap = 19,", common)


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
    for key, dtype in ARRAYS:
        assert got[key].dtype == dtype, (where, key, got[key].dtype)
        if not np.array_equal(got[key], np.asarray(exp[key], dtype=dtype)):
            bad = np.flatnonzero(got[key] != np.asarray(exp[key], dtype=dtype)) if len(got[key]) == len(exp[key]) else []
            raise AssertionError((where, key, len(got[key]), len(exp[key]), [(int(i), int(got[key][i]), int(exp[key][i])) for i in bad[:5]]))
    for key in ("data", "cut_data"):
        g = got[key] if isinstance(got[key], bytes) else got[key].tobytes()
        assert isinstance(got[key], bytes) or got[key].dtype == (np.uint8 if eb == 1 else np.int32), (where, key)
        if g != exp[key]:
            a, b = np.frombuffer(g, dtype=np.uint8), np.frombuffer(exp[key], dtype=np.uint8)
            n = min(len(a), len(b))
            raise AssertionError((where, key, len(a), len(b), np.flatnonzero(a[:n] != b[:n])[:5].tolist()))


def check(rows, where, eb=1, forms=(False, True), v=None, exp=None, utf8=False, **spec):
    """the rows (bytes each) through the host form and the tensor form against the model; -> (the model's answer, the
    statistics of the last call)"""
    v = v or handle()
    data, off = M.join(rows, eb)
    model_spec = {k: x for k, x in spec.items() if k != "hash_bits"}
    exp = exp or M.repeat_rows(data, off, elem_bytes=eb, utf8=utf8, **model_spec)
    st = None
    for tensor in forms:
        if tensor:
            got = v.repeat_rows_tensor(to_gpu(data, eb), off_gpu(off), mask=True, src=True, compact=True, cut=True, utf8=utf8, **spec)
        else:
            got = v.repeat_rows(np.frombuffer(data, dtype=np.uint8 if eb == 1 else np.int32), off, mask=True, src=True, compact=True, cut=True,
                                utf8=utf8, **spec)
        compare(got, exp, eb, (where, "tensor" if tensor else "host"), tensor)
        st = v.repeat_stats()
        assert {k: st[k] for k in exp["stats"]} == exp["stats"], (where, st, exp["stats"])
        if spec.get("scope", 0) == 0:
            assert st["n_repeats"] == st["n_windows"] - st["n_distinct"], (where, st)
    return exp, st


@pytest.mark.gpu
@pytest.mark.parametrize("eb", [1, 4])
def test_window_shapes_short_rows_and_empty_rows(eb):
    import torch
    rng = np.random.default_rng(10 + eb)
    v = handle()
    for k in (1, 2, 13, 63, 64):
        src = rng.integers(0, 4, 400)
        rows = [b"", b"", elems(src[5:5 + k - 1], eb), elems(src[5:5 + k], eb), elems(src[5:5 + k + 1], eb), b"", b"", b"",
                elems(rng.integers(0, 4, k + 30), eb), elems(src[:120 + k], eb), elems(src[100:100 + k], eb), b"", b""]
        for scope in (0, 1):
            exp, st = check(rows, ("shapes", k, scope), eb, ngram=k, scope=scope)
            assert exp["repeats"][2] == 0 and exp["repeats"][4] >= 1 and exp["repeats"][10] == 1, k
            assert st["n_windows"] == sum(max(len(r) // eb - k + 1, 0) for r in rows)
        check([elems(src[:3 * k + 7], eb)], ("one row", k), eb, ngram=k)
        check([b"", elems(src[:k - 1], eb), b""], ("no window", k), eb, ngram=k, forms=(True,))
        check([b"", b""], ("empty rows only", k), eb, ngram=k, forms=(True,))
    r = v.repeat_rows_tensor(to_gpu(b"", eb), off_gpu([0]), ngram=3, mask=True, src=True, compact=True, cut=True, utf8=False)  # an empty batch
    assert all(r[key].numel() == 0 for key, _ in ARRAYS[:8]) and r["row_off"].tolist() == [0] and r["cut_off"].tolist() == [0]
    assert r["cut_data"].numel() == 0 and r["cut_data"].dtype == (torch.uint8 if eb == 1 else torch.int32) and v.repeat_stats()["n_rows"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("eb,k", [(4, 1), (4, 2), (4, 13), (4, 63), (4, 64), (1, 13), (1, 64), (1, 2)])
def test_tile_and_halo_edges(eb, k):
    for tile in (T, G["tile"]):  # the tile of the key kernel, the tile of the flag and cover kernels
        for i, (start, src) in enumerate(K.edge_starts(tile, k)):
            rows, _, facts = K.edge_case(tile, k, eb, start, src)
            exp, _ = check(rows, ("tile edge", tile, eb, k, start, src), eb, ngram=k, forms=(False, True) if i == 0 else (True,))
            assert (k < 4 and eb == 1) or (exp["src"][start] == src and (eb == 1 or (exp["first_repeat"], exp["covered"]) == ([start], [k])))
        for shift in (-1, 0, 1):
            rows, _, facts = K.row_end_case(tile, k, eb, tile + shift)
            exp, _ = check(rows, ("row end", tile, eb, k, shift), eb, ngram=k, forms=(True,))
            assert (k < 4 and eb == 1) or exp["repeats"] == facts["repeats"]
    for n in (T, T + 1, 2 * T, G["tile"], G["tile"] + 1, 2 * G["tile"], G["cut"], G["cut"] + 1):
        rows, _, _ = K.sized_case(n, k, eb)
        for scope in (0, 1):
            check(rows, ("sized", n, eb, k, scope), eb, ngram=k, scope=scope, forms=(True,))


@pytest.mark.gpu
@pytest.mark.parametrize("eb", [1, 4])
def test_one_window_per_row_over_a_whole_tile(eb):
    rows, _, facts = K.unit_rows_case(T, 5, eb)
    exp, st = check(rows, ("unit rows", eb), eb, ngram=5)
    assert [i for i, x in enumerate(exp["repeats"]) if x] == facts["repeat_rows"] and st["n_windows"] == T and st["n_distinct"] == T // 2
    check(rows, ("unit rows, scope 1, kept", eb), eb, ngram=5, scope=1, max_repeats=1, forms=(True,))


@pytest.mark.gpu
@pytest.mark.parametrize("eb", [1, 4])
def test_periodic_row(eb):
    rows, _, _ = K.periodic_case(3000, eb)
    exp, st = check(rows, ("periodic", eb), eb, ngram=13)
    assert exp["src"][:3000 - 12] == [-1, -1] + [p % 2 for p in range(2, 3000 - 12)] and st["n_distinct"] == 2 and exp["covered"] == [2998]
    check(rows, ("periodic, earlier rows only", eb), eb, ngram=13, scope=1, forms=(True,))


_long = {}


def long_case():
    """the long-row case and the model's answer to it, computed once"""
    if not _long:
        rows, eb, facts = K.long_row_case()
        data, off = M.join(rows, eb)
        _long.update(rows=rows, facts=facts, exp=M.repeat_rows(data, off, elem_bytes=eb, ngram=13))
    return _long


@pytest.mark.gpu
def test_one_long_row_beside_short_ones():
    c = long_case()
    exp, st = check(c["rows"], "long row", 4, exp=c["exp"], ngram=13)
    long, block = c["facts"]["long"], c["facts"]["block"]
    assert exp["repeats"][long] == 3 * (block - 12) == exp["covered"][long] - 3 * 12 and exp["first_repeat"][long] == c["facts"]["at"][0]
    assert exp["repeats"][long + 1:] == [3] * 25 and exp["first_src_row"][long + 1:] == [long] * 25 and exp["kept"] == list(range(25))


@pytest.mark.gpu
@pytest.mark.parametrize("eb", [1, 4])
def test_multiplicity(eb):
    rows, _, _ = K.multiplicity_case(7, eb)
    exp, st = check(rows, ("multiplicity", eb), eb, ngram=7)
    assert exp["repeats"] == [0, 0, 999, 5, 5, 0, 1] and st["n_distinct"] == st["n_windows"] - 1010
    data, off = M.join(rows, eb)
    for e, s in enumerate(exp["src"]):  # src is always the smallest position that holds the window
        assert s < 0 or (s < e and data.find(data[e * eb:(e + 7) * eb]) == s * eb), (e, s)
    check(rows, ("multiplicity, earlier rows only", eb), eb, ngram=7, scope=1, forms=(True,))


@pytest.mark.gpu
@pytest.mark.parametrize("eb", [1, 4])
def test_key_collisions_change_nothing(eb):
    rng = np.random.default_rng(30 + eb)
    k = 6
    parts = [elems(rng.integers(0, 90, 40), eb) for _ in range(20)]  # 700 windows, nearly all distinct
    rows = parts + [parts[3][5 * eb:25 * eb], elems(rng.integers(0, 90, 100), eb), parts[7] + parts[8], b"", parts[11][2 * eb:(2 + k) * eb]]
    for scope in (0, 1):
        wide, st_wide = check(rows, ("64 bits", eb, scope), eb, ngram=k, scope=scope)
        narrow, st = check(rows, ("8 bits", eb, scope), eb, exp=wide, ngram=k, scope=scope, hash_bits=8)
        assert st["n_distinct"] >= 600 and st["n_collided"] > 0 and st_wide["n_collided"] == 0  # (more than 256 distinct windows on 256 keys)
    for bits in (9, 16, 33, 63):
        check(rows, (bits, eb), eb, exp=wide, ngram=k, scope=1, hash_bits=bits, forms=(True,))


@pytest.mark.gpu
@pytest.mark.parametrize("eb", [1, 4])
def test_dirty_bytes_behind_the_data_and_every_byte_phase(eb):
    import torch
    rng = np.random.default_rng(40 + eb)
    k = 5
    v = handle()
    for phase in range(4):
        base = elems(rng.integers(0, 3, 22), eb)
        rows = [elems(rng.integers(0, 3, phase), eb), base, elems(rng.integers(0, 3, 6), eb),
                elems(rng.integers(0, 3, 11), eb) + base[2 * eb:14 * eb] + elems(rng.integers(0, 3, 7), eb)]  # (a planted span: 8 repeats at least)
        n = sum(len(r) for r in rows)
        rows.append(elems(rng.integers(0, 3, (-n // eb) % 4 + 4), eb))  # (a whole number of words: the tensor is read where it lies, 0xff behind it)
        data, off = M.join(rows, eb)
        exp = M.repeat_rows(data, off, elem_bytes=eb, ngram=k)
        big = torch.full((len(data) // eb + 4096,), 0xff if eb == 1 else -1, dtype=torch.uint8 if eb == 1 else torch.int32, device="cuda")
        big[:len(data) // eb] = to_gpu(data, eb)
        got = v.repeat_rows_tensor(big[:len(data) // eb], off_gpu(off), ngram=k, mask=True, src=True, compact=True, cut=True, utf8=False)
        compare(got, exp, eb, ("dirty", eb, phase), True)
        assert sum(exp["repeats"]) >= 8 and {k_: v.repeat_stats()[k_] for k_ in exp["stats"]} == exp["stats"]


@pytest.mark.gpu
@pytest.mark.parametrize("eb", [1, 4])
def test_the_cut(eb):
    rows, _, facts = K.cut_case(6, eb, G["cut"])
    exp, st = check(rows, ("cut", eb), eb, ngram=6)
    assert all(exp["cut_off"][i] == exp["cut_off"][i + 1] for i in facts["empty"]) and st["n_cut_elems"] == exp["cut_off"][-1] > G["cut"]
    check(rows, ("cut, earlier rows only", eb), eb, ngram=6, scope=1, max_repeats=3, forms=(True,))
    # a batch that is covered but for the start of its first window (a constant row keeps one element at every k: every
    # window from the second on repeats the first; k - 1 elements stay where the row is k - 1 long and has no window)
    exp, st = check([elems(np.zeros(G["cut"] + 77, dtype=np.int64) + 9, eb)], ("all covered", eb), eb, ngram=6)
    assert st["n_cut_elems"] == 1 and exp["mask"][:3] == [0, 1, 1]
    exp, st = check([elems(np.zeros(5, dtype=np.int64) + 9, eb), elems(np.zeros(G["cut"], dtype=np.int64) + 9, eb)], ("k - 1 stay", eb), eb, ngram=6)
    assert st["n_cut_elems"] == 5 + 1 and exp["cut_off"] == [0, 5, 6]
    # nothing covered: the cut is the input
    flat = K.distinct(G["cut"] + 9, eb, 3)
    exp, st = check([b"".join(flat[:50]), b"".join(flat[50:])], ("nothing covered", eb), eb, ngram=6)
    assert st["n_covered"] == 0 and exp["cut_data"] == b"".join(flat)
    v = handle()
    data, off = M.join(rows, eb)
    only = v.repeat_rows_tensor(to_gpu(data, eb), off_gpu(off), ngram=6, cut=True, utf8=False)
    assert sorted(only) == ["covered", "cut_data", "cut_off", "first_repeat", "first_src_pos", "first_src_row", "repeats"]
    assert only["cut_data"].cpu().numpy().tobytes() == check(rows, "again", eb, ngram=6, forms=())[0]["cut_data"]


@pytest.mark.gpu
def test_scope_and_the_overlap_call():
    rng = np.random.default_rng(55)
    v = handle()
    k = 4
    shared = elems(rng.integers(0, 50, 12), 1)
    rows = [elems(rng.integers(50, 99, 20), 1), b"xyzxyzxyzxyz", shared + elems(rng.integers(50, 99, 6), 1), b"ababababab" + shared[3:10],
            elems(rng.integers(50, 99, 14), 1), shared[1:9] + b"xyzxyz"]
    any0, _ = check(rows, "scope 0", ngram=k, scope=0)
    earlier, _ = check(rows, "scope 1", ngram=k, scope=1)
    assert any0["repeats"][1] > 0 and earlier["repeats"][1] == 0  # what a row repeats of itself stays at scope 1
    assert earlier["repeats"][3] == 4 and any0["repeats"][3] > 4 and all(a >= b for a, b in zip(any0["repeats"], earlier["repeats"]))
    for i in range(6):  # repeats at scope 1 are the hits of the row against the rows in front of it
        data, off = M.join(rows[:i])
        hits = v.overlap_rows(rows[i], [0, len(rows[i])], data, off, ngram=k)["hits"] if rows[i] else np.zeros(1, dtype=np.int64)
        assert int(hits[0]) == earlier["repeats"][i], i


@pytest.mark.gpu
def test_utf8_flag():
    import torch
    docs, text = K.utf8_pair()
    rows = [d.encode("utf8") for d in docs]
    exp, _ = check(rows, "shared continuation byte, raw", ngram=len(text) + 1)
    assert exp["repeats"] == [0, 1]
    exp, _ = check(rows, "shared continuation byte", ngram=len(text) + 1, utf8=True)
    assert exp["repeats"] == [0, 0]
    exp, st = check(rows, "text behind the sign", ngram=len(text), utf8=True)
    assert exp["repeats"] == [0, 1] and exp["cut_data"].decode("utf8") == docs[0] + "é"
    exp, st = check(["xab©".encode("utf8"), "ab©".encode("utf8")], "ends inside a sequence", ngram=3, utf8=True)
    assert exp["repeats"] == [0, 1] and st["n_windows"] == 3
    check([b"\x80\x80ab\x80", b"\x80ab"], "invalid text", ngram=2, utf8=True)
    check([b"\x80\x80", b"\xa9\x80\x80"], "no eligible window", ngram=2, utf8=True)
    rng = np.random.default_rng(56)
    alphabet = ["a", "b", " ", "é", "中", "©", "\U0001f600"]
    lines = ["".join(alphabet[i] for i in rng.integers(0, len(alphabet), int(n))).encode("utf8") for n in rng.integers(0, 60, 80)]
    for k in (1, 2, 3, 5, 13):
        exp, _ = check(lines, ("random text", k), ngram=k, utf8=True, forms=(True,))
        assert exp["cut_data"].decode("utf8") is not None  # valid UTF-8 stays valid under the cut
    v = handle()
    assert v.repeat_rows(b"".join(lines), np.cumsum([0] + [len(x) for x in lines]), ngram=5, cut=True)["cut_data"] == \
        M.repeat_rows(b"".join(lines), np.cumsum([0] + [len(x) for x in lines]), ngram=5, utf8=True)["cut_data"]  # (utf8=None: on for text)
    ids = torch.arange(8, dtype=torch.int32, device="cuda")
    with pytest.raises(W.WordPieceError, match="flags"):
        v.repeat_rows_tensor(ids, off_gpu([0, 8]), ngram=2, utf8=True)
    assert W.lib().wp_last_error().startswith(b"repeat: flags")
    assert v.repeat_rows_tensor(ids, off_gpu([0, 8]), ngram=2)["repeats"].tolist() == [0]  # (utf8=None: off for ids)
    cut, covered = v.repeat_docs(["© all rights reserved, é", "b", "é all rights reserved, é"], ngram=12)
    assert cut == ["© all rights reserved, é", "b", "é"] and covered.tolist() == [0, 0, len(" all rights reserved, é\n".encode("utf8"))]


@pytest.mark.gpu
def test_bad_offsets_in_the_device_form_name_the_first_bad_row():
    import torch
    v = W.Vocab(VOCAB)
    data = to_gpu(b"abcdefgh" * 8, 1)
    for off, row in (([1, 2, 3], 0), ([0, 3, 2, 8], 1), ([0, 2, 4, 3], 2), ([0, 4, 2, 1], 1), ([-1, 2], 0), ([0, -1], 0), ([0, 2 ** 40, 3], 1)):
        with pytest.raises(W.WordPieceError) as e:
            v.repeat_rows_tensor(data, off_gpu(off), ngram=2, cut=True, compact=True)
        assert "row_off" in str(e.value) and str(e.value).endswith("row %d" % row), (off, str(e.value))
    r = v.repeat_rows_tensor(data, off_gpu([0, 4, 8, 20]), ngram=2)  # the handle works on
    assert r["repeats"].tolist() == [0, 0, 9] and torch.equal(r["first_src_row"].cpu(), torch.tensor([-1, -1, 0], dtype=torch.int32))


@pytest.mark.gpu
def test_handle_states():
    import torch
    import dedup_model as DM
    v = W.Vocab(VOCAB)
    assert v.repeat_stats()["n_rows"] == -1
    rng = np.random.default_rng(60)
    small = [b"abcabc", b"", b"xabcab"]
    large = [elems(rng.integers(0, 3, int(n)), 1) for n in rng.integers(0, 60, 3000)]
    check(small, "first call", v=v, ngram=3)
    check(small, "second call", v=v, ngram=3, scope=1, forms=(True,))
    text = ("b a b . 中 ab a b " * 40).encode("utf8")
    ids = v.encode(text)
    assert len(ids) == 9 * 40 and v.repeat_stats()["n_rows"] == -1  # (an encode since: as every layer's statistics)
    check(large, "grown", v=v, ngram=6, forms=(True,))
    d = v.dedup_rows(*DM.join(large), compact=True)
    assert d["kept"].tolist() == DM.dedup_rows(*DM.join(large))["kept"] and v.repeat_stats()["n_rows"] == 3000  # (each layer keeps its own)
    v.overlap_rows(b"abcd", [0, 4], b"bcd", [0, 3], ngram=2)
    check(small + [b""], "shrunk, behind a dedup and an overlap call", v=v, ngram=3, forms=(True,))
    assert v.encode(text).tolist() == ids.tolist() and v.repeat_stats()["n_rows"] == -1
    # views live until the handle's next call, whatever other handles do; the next call hands out arrays of its own
    data, off = M.join(large)
    dt, ot = to_gpu(data, 1), off_gpu(off)
    views = v.repeat_rows_tensor(dt, ot, ngram=6, mask=True, src=True, compact=True, cut=True, utf8=False, copy=False)
    kept = {k: x.clone() for k, x in views.items()}
    other = W.Vocab(["x", "b a"])
    other.repeat_rows_tensor(dt[:ot[40]], ot[:41], ngram=3, mask=True, src=True, compact=True, cut=True, utf8=False)
    other.encode(text)
    assert all(torch.equal(views[k], kept[k]) for k in views)
    copies = v.repeat_rows_tensor(dt, ot, ngram=6, mask=True, src=True, compact=True, cut=True, utf8=False)
    assert all(torch.equal(copies[k], kept[k]) for k in kept)
    v.repeat_rows_tensor(dt[:ot[40]], ot[:41], ngram=2, scope=1, cut=True, utf8=False)  # (a smaller call writes over the library's buffers ...)
    assert all(torch.equal(copies[k], kept[k]) for k in kept)                            # (... and the copies of the call before are no part of them)
    for rows, trim in ((small, False), (large[:700], False), ([b"q"], True), (large[:90], False)):
        if trim:
            v.trim()
        check(rows, ("sizes", len(rows), trim), v=v, ngram=6, forms=(trim,))


@pytest.mark.gpu
def test_stage_timing_fills_the_four_stages():
    v = W.Vocab(VOCAB)
    v.set_option(W.WP_OPT_STAGE_TIMING, 1)
    c = long_case()
    check(c["rows"], "timed", 4, v=v, exp=c["exp"], ngram=13, forms=(True,))
    s = v.stats()
    assert s["ms_sa"] > 0 and s["ms_scan"] > 0 and s["ms_walk"] > 0 and s["ms_decode"] > 0 and s["ms_normalize"] == 0
    assert abs(s["ms_total"] - (s["ms_decode"] + s["ms_sa"] + s["ms_scan"] + s["ms_walk"])) < 1e-3


@pytest.mark.gpu
def test_end_to_end_with_the_encoder_the_dedup_and_the_packer():
    import torch
    import dedup_model as DM
    vocab = ["[UNK]", "[CLS]", "[SEP]", "hello", "world", ",", "cafe", "##s", "a", "b", "the", "##x", "of", "and", "is", "in"]
    words = ["the", "world", "of", "cafes", "is", "in", "and", "hello", "a", "cafe", "b", ","]
    rng = np.random.default_rng(70)

    def line(n):
        return " ".join(words[i] for i in rng.integers(0, len(words), n))
    banner = line(14)
    docs = [line(int(n)) for n in rng.integers(5, 40, 120)]
    with_banner = [7, 30, 31, 90, 119]
    for d in with_banner:  # a templated line inside otherwise different documents, with changed case, accents and spacing
        docs[d] = line(3) + " " + banner.upper().replace("CAFE", "CAFÉ").replace(" ", "  ") + " " + line(4)
    docs[50] = docs[12]  # an equal row, which the exact dedup drops first
    v = W.Vocab(vocab, normalize=W.WP_NORM_BERT_UNCASED)
    text, off = W.join_docs(docs)
    t = torch.zeros((len(text) + 19) // 16 * 16, dtype=torch.uint8, device="cuda")
    t[:len(text)] = to_gpu(text, 1)
    ids, splits = v.encode_rows_tensor(t[:len(text)], torch.from_numpy(off).cuda())
    dd = v.dedup_rows_tensor(ids, splits, compact=True)
    got = v.repeat_rows_tensor(dd["data"], dd["row_off"], ngram=8, mask=True, src=True, compact=True, cut=True)
    # the same chain on the host, with the models
    hd = DM.dedup_rows(ids.cpu().numpy().tobytes(), splits.tolist(), elem_bytes=4)
    assert hd["kept"] == [i for i in range(120) if i != 50]
    exp = M.repeat_rows(hd["data"], hd["row_off"], elem_bytes=4, ngram=8)
    compare(got, exp, 4, "ids of the rows call, deduplicated", True)
    dirty = [hd["kept"].index(d) for d in with_banner[1:]]
    assert [i for i, r in enumerate(exp["repeats"]) if r] == dirty and exp["first_src_row"][dirty[0]] == hd["kept"].index(7)
    packed = v.pack_sequences_tensor(got["cut_data"], got["cut_off"], max_len=128)
    assert int(packed["lengths"].sum()) == int(got["cut_off"][-1]) == exp["cut_off"][-1] == exp["stats"]["n_elems"] - exp["stats"]["n_covered"]


@pytest.mark.gpu
def test_random_parity():
    rng = np.random.default_rng(80)
    v = handle()
    for it in range(60):
        eb = 1 if it % 2 else 4
        k = (1, 2, 3, 13, 64)[it % 5]
        alphabet = int(rng.integers(2, 5))
        n_rows = int(rng.integers(1, 40))
        lens = rng.integers(0, max(2, 4000 // n_rows), n_rows) if it % 3 else rng.integers(0, 3 * k + 2, n_rows)
        rows = [elems(rng.integers(0, alphabet, int(n)), eb) for n in lens]
        if it % 4 == 0 and k >= 13:  # (long windows over a small alphabet seldom repeat by themselves: plant some)
            rows += [rows[0][:len(rows[0]) // (2 * eb) * eb] + rows[-1], rows[0]]
        check(rows, ("random", it, eb, k), eb, v=v, ngram=k, scope=it // 5 % 2, max_repeats=int(rng.integers(0, 4)), hash_bits=(0, 8, 12)[it % 3],
              forms=(it % 2 == 0, True))


@pytest.mark.gpu
@pytest.mark.parametrize("lib_name,guard", [("libwordpiece_amd_dbg.so", "0"), ("libwordpiece_amd.so", "1")])
def test_hardened_runs(tmp_path, lib_name, guard):
    """(a fresh child: once on the bounds-checking build, once with WP_ARENA_GUARD=1) the tile-edge, the collision, the
    cut and the long-row cases: no gather or store outside an array (kSiteRepeat, kSiteOverlap, kSiteGroup), no guard zone
    of the call's arenas overwritten"""
    lib = os.path.join(PKG, lib_name)
    assert os.path.exists(lib), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "repeat_hard_run.py"
    script.write_text('''
import sys
import torch  # (before the library, as tests/conftest.py: the HIP runtime loaded first serves the process)
sys.path.insert(0, %r); sys.path.insert(0, %r)
import wordpiece_amd as W
import test_gpu_repeat as T
v = T.handle()
v.encode("ab a")
assert v.stats()["reserved0"] == %d, "not the build this run is about"
for eb, k in ((4, 1), (4, 13), (4, 64), (1, 13), (1, 64)):
    T.test_tile_and_halo_edges(eb, k)
T.test_window_shapes_short_rows_and_empty_rows(1)
T.test_one_window_per_row_over_a_whole_tile(1)
T.test_key_collisions_change_nothing(4)
T.test_the_cut(1)
T.test_the_cut(4)
T.test_utf8_flag()
T.test_one_long_row_beside_short_ones()
print("REPEAT_HARD_OK")
''' % (os.path.dirname(PKG), HERE, 1 if "dbg" in lib_name else 0))
    env = dict(os.environ, WP_LIB=lib, WP_ARENA_GUARD=guard)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "REPEAT_HARD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
