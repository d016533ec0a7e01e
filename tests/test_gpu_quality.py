"""GPU checks of the quality signals (wp_quality_rows, wp_quality_rows_device) against tests/quality_model.py, exactly:
the signals, the reasons, the kept rows, the compact form, each with its dtype, and the statistics — with words, lines,
dot runs and characters of every length across every tile edge and every row boundary, empty and one-byte rows, one long
row beside a thousand short ones, lines of spaces, permuted rows, duplicate lines of every kind, every rule at equality
and one past it, both presets, bytes behind the data, bad offsets, the empty batch, across the states of a handle and end
to end with the exact dedup and the encoder."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import quality_cases as K
import quality_model as M
import wordpiece_amd as W

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")
VOCAB = ["[UNK]", "a", "b", "##b", "the", "of", "."]
T = K.T
STOP = [b"the", b"of", b"a"]
RULE_FORMS = [("text_words", None, "under"), ("text_words", None, "over"), ("text_word_chars", "text_words", "under"),
              ("text_word_chars", "text_words", "over"), ("hashes", "words", "over"), ("ellipses", "words", "over"), ("bullet_lines", "lines", "over"),
              ("ellipsis_lines", "lines", "over"), ("alpha_words", "words", "under"), ("stop_words", None, "under"), ("dup_lines", "lines", "over"),
              ("dup_line_chars", "chars", "over"), ("terminal_lines", "lines", "under"), ("short_lines", "lines", "over"), ("newlines", "words", "over")]


def test_geometry_matches_the_kernels():
    src = open(os.path.join(PKG, "csrc", "quality.h")).read()
    common = open(os.path.join(PKG, "csrc", "common.h")).read()
    dedup = open(os.path.join(PKG, "csrc", "dedup.h")).read()
    block = int(re.search(r"constexpr int kBlock = (\d+);", common).group(1))
    items = int(re.search(r"constexpr int kQualItems = (\d+);", src).group(1))
    assert re.search(r"constexpr int kQualTile = kBlock \* kQualItems;", src) and K.T == block * items
    assert K.SLOTS == int(re.search(r"constexpr int kQualSlots = (\d+);", src).group(1))
    assert re.search(r"constexpr \w+ kDedupChunk\w* = %d;" % K.CHUNK, dedup), "the chunk of the duplicate-row search"
    assert re.search(r"kSiteQuality = 22,", common) and re.search(r"kBoundSites = 23", common) and re.search(r"kSiteGroup = 21,", common)


_handle = []


def handle():
    if not _handle:
        _handle.append(W.Vocab(VOCAB))
    return _handle[0]


def to_gpu(data):
    import torch
    if not data:
        return torch.zeros(0, dtype=torch.uint8, device="cuda")
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def off_gpu(off):
    import torch
    return torch.tensor(np.asarray(off).tolist(), dtype=torch.int64, device="cuda")


def compare(got, exp, where, tensor):
    """every array of one call against the model's, dtype included"""
    if tensor:
        got = {k: x.cpu().numpy() for k, x in got.items()}
        assert got["reasons"].dtype == np.int32
        got["reasons"] = got["reasons"].view(np.uint32)
    n = len(exp["reasons"])
    for key, dtype, want in (("signals", np.int64, np.asarray(exp["signals"], dtype=np.int64).reshape(23, n)), ("reasons", np.uint32, exp["reasons"]),
                             ("kept", np.int32, exp["kept"]), ("row_off", np.int64, exp["row_off"])):
        want = np.asarray(want, dtype=dtype)
        assert got[key].dtype == dtype and got[key].shape == want.shape, (where, key, got[key].dtype, got[key].shape, want.shape)
        if not np.array_equal(got[key], want):
            bad = np.argwhere(got[key] != want)[:6]
            raise AssertionError((where, key, [(tuple(int(x) for x in i), int(got[key][tuple(i)]), int(want[tuple(i)])) for i in bad],
                                  [M.SIGNALS[int(i[0])] for i in bad] if key == "signals" else None))
    g = got["data"] if isinstance(got["data"], bytes) else got["data"].tobytes()
    assert g == exp["data"], (where, "data", len(g), len(exp["data"]))


def check(rows, where, forms=(False, True), v=None, rules=None, stop=STOP, short=0, dup=True, exp=None):
    """the rows through the host form and the tensor form against the model -> the model's answer"""
    v = v or handle()
    data, off = K.join(rows)
    rules = dict(rules or {})
    exp = exp or M.quality(data, off.tolist(), limit=M.limits(**rules), stop_words=stop, short_line_chars=short, dup_lines=dup)
    for tensor in forms:
        if tensor:
            got = v.quality_rows_tensor(to_gpu(data), off_gpu(off), rules=rules, stop_words=stop, short_line_chars=short, dup_lines=dup, compact=True)
        else:
            got = v.quality_rows(data, off, rules=rules, stop_words=stop, short_line_chars=short, dup_lines=dup, compact=True)
        compare(got, exp, (where, "tensor" if tensor else "host"), tensor)
        assert v.quality_stats() == exp["stats"], (where, v.quality_stats(), exp["stats"])
    return exp


_seen = np.zeros(23, dtype=bool)


def note(exp):
    _seen[:] |= np.asarray(exp["signals"]).reshape(23, -1).any(axis=1)
    return exp


@pytest.mark.gpu
def test_every_tile_edge_of_a_long_row():
    rows = K.tile_edge_rows()
    exp = note(check(rows, "tile edges", rules={"max_ellipsis_per_word": 0}))
    assert min(exp["signals"][M.S["invalid"]]) == 0 < max(exp["signals"][M.S["invalid"]]) and 0 < len(exp["kept"]) < len(rows)
    one = check(rows[7:8], "one row of 3 T bytes", forms=(True,))  # (every tile inside one row: the sums of a tile meet in one slot)
    assert one["signals"][M.S["bytes"]] == [3 * T]


@pytest.mark.gpu
def test_every_row_boundary_at_every_byte_phase():
    rows = K.row_boundary_rows()
    note(check(rows, "row boundaries"))
    note(check([b"x"] + rows, "row boundaries, shifted by one byte", forms=(True,)))  # (the other phase of the aligned words)
    note(check(rows[::-1], "row boundaries, reversed", forms=(True,)))


@pytest.mark.gpu
def test_empty_rows_and_rows_of_one_byte():
    note(check(K.empty_and_single_rows(), "empty and single", rules={"min_text_words": 1}))
    check([b""] * 5, "only empty rows in the tensor form", forms=(True,), rules={"min_text_words": 1})
    check([b"", b"a", b""], "one byte in all", rules={"max_text_words": 0})


@pytest.mark.gpu
def test_one_long_row_beside_a_thousand_short_ones():
    rows = K.long_beside_short(np.random.default_rng(5))
    assert len(rows) == 1001 and len(rows[500]) == 3 * T + 5
    exp = note(check(rows, "long beside short", rules={"min_text_words": 2}))
    assert exp["signals"][M.S["bytes"]][500] == 3 * T + 5 and 0 < exp["stats"]["n_kept"] < 1001


@pytest.mark.gpu
def test_lines_of_spaces_only():
    exp = note(check(K.space_lines_rows(), "space lines", rules={"min_terminal_lines": 1}))
    assert exp["signals"][M.S["lines"]] == [3, 3, 0, 1, 3] and exp["signals"][M.S["terminal_lines"]] == [0] * 5


@pytest.mark.gpu
def test_row_permutation_leaves_every_rows_signals():
    rng = np.random.default_rng(6)
    rows = K.row_boundary_rows()[:120] + K.duplicate_rows() + K.tile_edge_rows()[:3]
    base = check(rows, "identity", forms=(True,))
    perm = rng.permutation(len(rows))
    got = handle().quality_rows_tensor(*[f(x) for f, x in zip((to_gpu, off_gpu), K.join([rows[i] for i in perm]))], stop_words=STOP, dup_lines=True)
    sig = got["signals"].cpu().numpy()
    assert np.array_equal(sig, np.asarray(base["signals"], dtype=np.int64)[:, perm])


@pytest.mark.gpu
def test_duplicate_lines():
    rows = K.duplicate_rows()
    exp = note(check(rows, "duplicate lines", rules={"max_dup_lines": 300, "max_dup_line_chars": 200}))
    assert exp["signals"][M.S["dup_lines"]] == [0, 0, 2, 1, 1, 1, 2, 0, 2, 0, 0, 1]
    assert exp["signals"][M.S["dup_line_chars"]][8] == 3 + 2 and exp["stats"]["n_dup_lines"] == 10
    off = check(rows, "without the stage", dup=False, forms=(True,))
    assert off["signals"][M.S["dup_lines"]] == [0] * len(rows) and off["signals"][:21] == exp["signals"][:21]
    check([b"a\na", b"a\na", b"a", b"\n", b""], "equal rows of duplicate lines")


def _corpus():
    return K.corpus(np.random.default_rng(7))


@pytest.mark.gpu
@pytest.mark.parametrize("r", range(15))
def test_every_rule_alone_at_equality_and_one_past(r):
    rows = _corpus()
    data, off = K.join(rows)
    sig = M.quality(data, off.tolist(), stop_words=STOP)["signals"]
    num, den, side = RULE_FORMS[r]
    pick = None
    for i in range(len(rows)):
        a, b = sig[M.S[num]][i], (sig[M.S[den]][i] if den else 1)
        L = a if den is None else (a * 1000 // b if b and a * 1000 % b == 0 else None)
        if L is not None and L >= 1 and L + 1 <= 10 ** 9 and (den is None or a > 0):
            pick = (i, L)
            break
    assert pick, "the corpus has no row at equality for rule %d" % r
    i, L = pick
    name = M.RULES[r]
    at = check(rows, ("rule", name, "at equality"), rules={name: L}, forms=(True,))
    past = check(rows, ("rule", name, "one past"), rules={name: L + 1 if side == "under" else L - 1}, forms=(r % 2 == 0, True))
    assert at["reasons"][i] == 0 and past["reasons"][i] == 1 << r
    assert all(x in (0, 1 << r) for x in at["reasons"] + past["reasons"]) and at["stats"]["rule_failed"][r] == sum(1 for x in at["reasons"] if x)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gopher", "fineweb"])
def test_presets(name):
    rows = _corpus()
    long_prose = (" ".join(["the quality of that model and the corpus have to be with the filter"] * 6) + ".\n").encode() * 3
    rows = rows + [long_prose, long_prose.replace(b"\n", b" ") + b"\n" + b"A second line of the document that ends well.\n"]
    rules = W.quality_rules(name)
    stop = [w.encode() for w in rules.pop("stop_words", ())]
    exp = note(check(rows, ("preset", name), rules=rules, stop=stop))
    assert 0 < exp["stats"]["n_kept"] < len(rows) and sum(1 for x in exp["stats"]["rule_failed"] if x) >= 3
    docs, reasons = handle().quality_docs([r.decode("utf8") for r in rows], rules=name)
    assert reasons.tolist() == exp["reasons"] and docs == [rows[k].decode("utf8") for k in exp["kept"]]


@pytest.mark.gpu
def test_every_signal_was_non_zero_in_some_case():
    for rows in (K.tile_edge_rows()[:8], K.duplicate_rows(), _corpus()):  # (the cases above, where this test runs alone)
        data, off = K.join(rows)
        note(M.quality(data, off.tolist(), stop_words=STOP))
    assert _seen.all(), [M.SIGNALS[k] for k in np.flatnonzero(~_seen)]
    exp = check(K.tile_edge_rows()[:8] + K.duplicate_rows() + _corpus(), "all signals", forms=(True,), short=5)
    assert all(any(row) for row in exp["signals"])


@pytest.mark.gpu
def test_dirty_bytes_behind_the_data():
    import torch
    rows = K.row_boundary_rows()[:60] + [("é" * 9).encode()[:-1]]
    data, off = K.join(rows)
    exp = M.quality(data, off.tolist(), stop_words=STOP)
    v = handle()
    for pad in (b"\xa9 the of...\n", b"\xff" * 16, b"\n\n\n\n", b"\x80\x80\x80 a"):
        buf = to_gpu(data + pad * 8)
        got = v.quality_rows_tensor(buf[:len(data)], off_gpu(off), stop_words=STOP, dup_lines=True, compact=True)
        compare(got, exp, ("dirty", pad), True)
        assert torch.equal(buf[len(data):].cpu(), torch.frombuffer(bytearray(pad * 8), dtype=torch.uint8))


@pytest.mark.gpu
def test_bad_offsets_in_the_device_form_name_the_first_bad_row():
    v = W.Vocab(VOCAB)
    data = to_gpu(b"abcdefgh" * 8)
    for off, row in (([1, 2, 3], 0), ([0, 3, 2, 8], 1), ([0, 2, 4, 3], 2), ([0, 4, 2, 1], 1), ([-1, 2], 0), ([0, -1], 0), ([0, 2 ** 40, 3], 1)):
        with pytest.raises(W.WordPieceError) as e:
            v.quality_rows_tensor(data, off_gpu(off), dup_lines=True, compact=True)
        assert "row_off" in str(e.value) and str(e.value).endswith("row %d" % row), (off, str(e.value))
    r = v.quality_rows_tensor(data, off_gpu([0, 4, 8, 20]))  # the handle works on
    assert r["signals"][M.S["words"]].tolist() == [1, 1, 1]


@pytest.mark.gpu
def test_the_empty_batch():
    import torch
    v = W.Vocab(VOCAB)
    got = v.quality_rows_tensor(to_gpu(b""), off_gpu([0]), rules={"min_text_words": 1}, compact=True)
    assert got["signals"].shape == (23, 0) and got["reasons"].numel() == 0 and got["kept"].numel() == 0 and got["data"].numel() == 0
    assert got["row_off"].tolist() == [0] and got["signals"].dtype == torch.int64 and v.quality_stats()["n_rows"] == 0
    check([], "no row in the host form", forms=(False,), v=v)
    check([b"", b""], "rows without bytes in both forms", v=v, rules={"min_text_words": 1})
    check([b"", b""], "rows without bytes, all kept", v=v)


@pytest.mark.gpu
def test_the_compact_form_feeds_the_dedup_and_the_encoder():
    import torch
    import dedup_model as DM
    docs = [b"the a of b.\n", b"# # #\n", b"the a of b.\n", b"b of the a!\nthe of.\n", b"...\n", b"a b\n"]
    v = W.Vocab(VOCAB)
    data, off = K.join(docs)
    rules = {"min_stop_words": 1, "max_hash_per_word": 500}
    exp = M.quality(data, off.tolist(), limit=M.limits(**rules), stop_words=STOP)
    assert exp["kept"] == [0, 2, 3, 5]
    q = v.quality_rows_tensor(to_gpu(data), off_gpu(off), rules=rules, stop_words=STOP, compact=True, copy=False)
    compare({k: x.clone() for k, x in q.items()}, exp, "compact views", True)
    ids, splits = v.encode_rows_tensor(q["data"].clone(), q["row_off"].clone())
    for k, i in enumerate(exp["kept"]):
        assert ids[splits[k]:splits[k + 1]].tolist() == v.encode(docs[i]).tolist(), i
    q = v.quality_rows_tensor(to_gpu(data), off_gpu(off), rules=rules, stop_words=STOP, compact=True)
    dd = v.dedup_rows_tensor(q["data"], q["row_off"], compact=True)
    hd = DM.dedup_rows(exp["data"], exp["row_off"])
    assert dd["kept"].tolist() == hd["kept"] == [0, 2, 3] and bytes(dd["data"].cpu().numpy()) == hd["data"] and dd["row_off"].tolist() == hd["row_off"]
    packed = v.pack_sequences_tensor(*v.encode_rows_tensor(dd["data"], dd["row_off"]), max_len=16)
    assert int(packed["lengths"].sum()) == sum(len(v.encode(docs[i])) for i in (0, 3, 5))
    assert torch.equal(q["kept"].cpu(), torch.tensor(exp["kept"], dtype=torch.int32))


@pytest.mark.gpu
def test_handle_states():
    import dedup_model as DM
    v = W.Vocab(VOCAB)
    assert v.quality_stats()["n_rows"] == -1 and v.dedup_stats()["n_rows"] == -1
    small = K.duplicate_rows()
    large = K.long_beside_short(np.random.default_rng(8))
    check(small, "first call", v=v, rules={"max_dup_lines": 300})
    assert v.dedup_stats()["n_rows"] == -1  # (the duplicate-row search inside left the dedup layer's statistics alone)
    text = ("b a b . the ab a b " * 40).encode("utf8")
    ids = v.encode(text)
    assert v.quality_stats()["n_rows"] == -1  # (an encode since: as every layer's statistics)
    check(large, "grown", v=v, forms=(True,), rules={"min_text_words": 2})
    d = v.dedup_rows(*DM.join(small), compact=True)
    mine = v.dedup_stats()
    assert d["kept"].tolist() == DM.dedup_rows(*DM.join(small))["kept"] and mine["n_rows"] == len(small) and v.quality_stats()["n_rows"] == 1001
    check(small + [b""], "shrunk, behind a dedup call", v=v, forms=(True,), rules={"max_dup_line_chars": 10})
    assert v.dedup_stats() == mine and v.encode(text).tolist() == ids.tolist() and v.quality_stats()["n_rows"] == -1
    v.trim()
    check(small[:3], "behind a trim", v=v)


@pytest.mark.gpu
def test_stage_timing_fills_the_four_stages():
    v = W.Vocab(VOCAB)
    v.set_option(W.WP_OPT_STAGE_TIMING, 1)
    check(K.duplicate_rows() + K.tile_edge_rows()[:4], "timed", v=v, forms=(True,), rules={"max_dup_lines": 300})
    s = v.stats()
    assert s["ms_sa"] > 0 and s["ms_scan"] > 0 and s["ms_walk"] > 0 and s["ms_decode"] > 0 and s["ms_normalize"] == 0
    assert abs(s["ms_total"] - (s["ms_decode"] + s["ms_sa"] + s["ms_scan"] + s["ms_walk"])) < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("lib_name,guard", [("libwordpiece_amd_dbg.so", "0"), ("libwordpiece_amd.so", "1")])
def test_hardened_runs(tmp_path, lib_name, guard):
    """(a fresh child: once on the bounds-checking build, once with WP_ARENA_GUARD=1) the tile-edge, row-boundary, long-row
    and duplicate-line cases: no gather or store outside an array (kSiteQuality, kSiteOverlap, kSiteDedup, kSiteGroup), no
    guard zone of the call's arenas overwritten"""
    lib = os.path.join(PKG, lib_name)
    assert os.path.exists(lib), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "quality_hard_run.py"
    script.write_text('''
import sys
import torch  # (before the library, as tests/conftest.py: the HIP runtime loaded first serves the process)
sys.path.insert(0, %r); sys.path.insert(0, %r)
import wordpiece_amd as W
import test_gpu_quality as T
v = T.handle()
v.encode("ab a")
assert v.stats()["reserved0"] == %d, "not the build this run is about"
T.test_every_tile_edge_of_a_long_row()
T.test_every_row_boundary_at_every_byte_phase()
T.test_empty_rows_and_rows_of_one_byte()
T.test_one_long_row_beside_a_thousand_short_ones()
T.test_duplicate_lines()
T.test_the_empty_batch()
T.test_presets("gopher")
print("QUALITY_HARD_OK")
''' % (os.path.dirname(PKG), HERE, 1 if "dbg" in lib_name else 0))
    env = dict(os.environ, WP_LIB=lib, WP_ARENA_GUARD=guard)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "QUALITY_HARD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
