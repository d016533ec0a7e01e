"""CPU checks of rows_cases.py: the Python models prove every claim with nothing of the code under test.

For every case: the byte position of every placed newline, the length of the text modulo a chunk and modulo a line tile, the
open end, where a 0x8A stands and that it ends no row, the id index of every placed row boundary (the model's row_splits), the
number of empty rows, of ids and of rows, the rows that normalise to nothing, the source and the normalised line tiles; that
the vocabulary is on the joined route (test_gpu_rows._expected_route); and the premise of that route, for every text the GPU
file passes: one encode of the joined text, cut at the document starts, is the per-document encode (rows_model.
encode_rows_joined == the expected rows; for a normalised handle in the normalised text, whose join is the normalised join).

Wall time (measured on the build container): see rows_cases.py."""
import bisect

import pytest

import normalize_model as NM
import offsets_model as OM
import rows_cases as K
import rows_model as R
from test_gpu_rows import _expected_route

T, RT, CHUNK = K.T, K.RT, K.CHUNK


def test_constants_and_table():
    """the constants come from the headers, every named case stands in the table of the module's docstring, and the subset of
    the bounds-checking build holds a case of every family"""
    assert (K.CHUNK, K.ITER, K.T, K.RT, K.ROW) == (16, 4096, 16384, 2048, 1024)
    doc = K.__doc__
    for name in K.names():
        parts = name.replace("_f1", "_f<F>").replace("_f4", "_f<F>").replace("_f7", "_f<F>").split("_")
        assert name in doc or any("_".join(parts[:k]) in doc for k in range(len(parts), 1, -1)), name
    assert all(n in K.names() for n in K.SUBSET) and {n[0] for n in K.SUBSET} == set("LSBNC")
    assert all(m in K.MAX_LENS for m in K.SUBSET_MAX_LENS)
    assert _expected_route(K.PLAIN) == 1 and _expected_route(K.NORM) == 1
    assert len(set(K.PLAIN)) == len(K.PLAIN) and len(set(K.NORM)) == len(K.NORM)
    for f in K.FLAG_SETS:   # DROP[f] holds only what the flag set drops, and the separator stays what it is
        assert NM.normalize(K.DROP[f], f)[0] == b"" and NM.normalize("\n", f)[0] == b"\n", f
    assert [len(w.encode()) for w in K.WIDE] == [2, 3, 4]
    assert "Ċ".encode()[-1] == 0x8A and "亊".encode()[-1] == 0x8A


def cdiv(a, b):
    return -(-a // b)


def gallop_probes(byte_of, b):
    """the entries cp_at_byte reads on its way down (rows.h): from min(b, n_text), steps of 1, 2, 4, ... until one lies in
    front of b"""
    hi, step, out = min(b, len(byte_of)), 1, []
    while hi > 0:
        q = hi - step if hi > step else 0
        out.append(q)
        if byte_of[q] < b:
            break
        hi = q
        step *= 2
    return out


def check_premise(c):
    """for every text the GPU file passes: the rows cut out of one encode of the joined text are the expected rows"""
    for label, t, starts, rows in c.runs():
        assert rows == R.split_lines(t), (c.name, label)
        if starts is not None:
            assert starts[0] == 0 and starts[-1] == len(t) and all(t[s - 1] == 0x0A for s in starts[1:]), (c.name, label)
        if c.flags == 0:
            m = K.model(tuple(c.vocab))
            for unit in (None, "byte", "char"):
                assert R.encode_rows_joined(m, rows, unit) == K.expected(c, rows, unit), (c.name, label, unit)
        else:
            m = K.model(tuple(c.vocab))
            normed = [NM.normalize(r, c.flags)[0] for r in rows]
            assert NM.normalize(R.join_docs(rows)[0], c.flags)[0] == R.join_docs(normed)[0], (c.name, label)
            assert not any(b"\n" in d for d in normed), (c.name, label)
            want = K.expected(c, rows, None)
            assert R.encode_rows_joined(m, normed)[:2] == want[:2] == R.encode_rows(m, normed)[:2], (c.name, label)


def check_case(name):
    c = K.build(name)
    data, vocab, mode, cl = c
    text = c.text
    assert _expected_route(vocab) == 1, name
    rows = R.split_lines(text)
    ids, splits, offs = K.expected(c, rows, "byte")
    assert K.expected(c, rows, "char")[:2] == (ids, splits) and K.expected(c, rows, None) == (ids, splits, None), name
    nl = [i for i, b in enumerate(text) if b == 0x0A]
    open_end = not text.endswith(b"\n")
    assert len(rows) == len(nl) + (1 if open_end and text else 0), name   # every '\n' ends a row, and nothing else does
    known = {"len", "len_mod16", "len_mod_tile", "newlines", "open_end", "newline_bytes_of_chunk", "empty_rows", "byte_0x8a",
             "n_ids", "n_rows", "splits_at", "start_minus_cp", "start_above_n_text", "unk_first_rows", "tile_inside_row",
             "dropped_rows", "front_delta", "src_tiles", "norm_tiles", "newline_at", "min_tiles", "probe_hit"}
    assert set(cl) <= known, (name, set(cl) - known)
    if "len" in cl:
        assert (len(text), len(text) % CHUNK, len(text) % T) == (cl["len"], cl["len_mod16"], cl["len_mod_tile"]), name
        assert nl == cl["newlines"] and open_end == cl["open_end"], (name, nl[:20])
    if "newline_bytes_of_chunk" in cl:
        assert sorted({p % CHUNK for p in nl}) == cl["newline_bytes_of_chunk"], name
    if "newline_at" in cl:
        assert all(text[p] == 0x0A for p in cl["newline_at"]), name
    if "byte_0x8a" in cl:
        for p in cl["byte_0x8a"]:
            assert text[p] == 0x8A and p % CHUNK == CHUNK - 1 and ("tile" not in name or p % T == T - 1), (name, p)
            assert p + 1 == len(text) or text[p + 1] == 0x0A, (name, p)
            first = p - (1 if "cp2" in name or "open" in name else 2 if "cp3" in name else 0)
            assert text[first - 1] in (0x0A, 0x20), (name, p)
            assert ("lone" in name) == (len(OM.decode_with_starts(text[first:p + 1])[0]) == 0), name
    if "empty_rows" in cl:
        assert sum(1 for r in range(len(rows)) if splits[r] == splits[r + 1]) == cl["empty_rows"], name
    if "n_ids" in cl:
        assert len(ids) == cl["n_ids"], (name, len(ids))
    if "n_rows" in cl:
        assert len(rows) == cl["n_rows"], (name, len(rows))
    for k in cl.get("splits_at", ()):
        assert k in splits[1:], (name, k)
    if "start_minus_cp" in cl:
        cps, bstarts = OM.decode_with_starts(text)
        p = bisect.bisect_left(bstarts, c.starts[1])
        assert c.starts[1] - p == cl["start_minus_cp"] and int(c.starts[1] > len(cps)) == cl["start_above_n_text"], name
    if "probe_hit" in cl:   # a probe of the gallop reads the answer's own entry
        cps, bstarts = OM.decode_with_starts(text)
        probes = gallop_probes(bstarts, c.starts[1])
        p = bisect.bisect_left(bstarts, c.starts[1])
        assert bstarts[p] == c.starts[1] and p in probes[:-1] and len(probes) >= 2, (name, p, probes)
        assert int(c.starts[1] > len(cps)) == cl["start_above_n_text"], name
    if name.startswith("B_"):   # the byte base and the code-point base of every row behind the first differ
        cps, bstarts = OM.decode_with_starts(text)
        assert all(s > bisect.bisect_left(bstarts, s) for s in c.starts[1:]), name
        assert len(ids) > RT - 2, name
    for r in cl.get("unk_first_rows", ()):
        assert ids[splits[r]] == vocab.index("[UNK]") and offs[splits[r]][0] == 0 and offs[splits[r]][1] >= 1, (name, r)
    if "tile_inside_row" in cl:
        t = cl["tile_inside_row"]
        assert any(splits[r] < t * RT and splits[r + 1] > (t + 1) * RT for r in range(len(rows))), name
    for r in cl.get("dropped_rows", ()):
        assert rows[r] and NM.normalize(rows[r], c.flags)[0] == b"" and splits[r] == splits[r + 1], (name, r)
    if "front_delta" in cl:
        d = len(NM.normalize(rows[0], c.flags)[0]) - len(rows[0])
        assert d == cl["front_delta"] and (d == 0 or abs(d) > CHUNK), (name, d)
    if "src_tiles" in cl:
        norm = NM.normalize(text, c.flags)[0]
        assert (cdiv(len(text), T), cdiv(len(norm), T)) == (cl["src_tiles"], cl["norm_tiles"]), name
        assert len(ids) > RT, name
    if "min_tiles" in cl:
        assert cdiv(len(text), T) >= cl["min_tiles"] and len(ids) > 3 * RT, name
    if name.startswith("N_only_dropped_all_1"):   # its open end is the text that normalises to nothing
        assert NM.normalize(text[:-1], c.flags)[0] == b"" and len(text) > 1, name
    if name.startswith("N_only_dropped_last"):    # its open end has a last line that normalises to nothing
        assert NM.normalize(text[:-1], c.flags)[0].endswith(b"\n"), name
    check_premise(c)


@pytest.mark.parametrize("name", K.names())
def test_rows_case(name):
    check_case(name)


def test_families_reach_their_edges():
    """what a family as a whole has to bring"""
    lens = {len(K.build(n).text) for n in K.names("L")}
    assert {1, 15, 16, 17, 32, T - 1, T, T + 1, 2 * T} <= lens
    opens = {len(K.build(n).text) for n in K.names("L") if not K.build(n).text.endswith(b"\n")}
    assert {1, 15, 16, 17, 32, T - 1, T, T + 1, 2 * T} <= opens
    assert {K.build(n).claims["n_rows"] for n in K.names("S") if n.startswith("S_rows")} == {255, 256, 257}
    assert {K.build("B_bound_%d" % k).claims["splits_at"][1] for k in (2047, 2048, 2049, 4095, 4096)} == {2047, 2048, 2049, 4095, 4096}
    assert K.build("S_behind_5000_4").claims["start_above_n_text"] == 1 and K.build("S_behind_5_2").claims["start_above_n_text"] == 0


@pytest.mark.parametrize("max_len", K.MAX_LENS)
def test_pack_batches(max_len):
    """family P: the combinations of specials that fit, the five row counts around the rows of a workgroup, and in every batch
    of five rows or more the five row lengths around what a row keeps"""
    lanes = K.lanes_for(max_len)
    assert lanes in (4, 8, 16, 32, 64) and (lanes >= max_len or lanes == 64) and (lanes == 4 or lanes // 2 < max_len)
    r = K.BLOCK // lanes
    batches = K.pack_batches(max_len)
    combos = {(cls_id, sep_id) for cls_id, sep_id, _ in batches}
    assert len(combos) == (4 if max_len >= 2 else 3) and (max_len >= 2 or (K.CLS, K.SEP) not in combos)
    m = K.model(tuple(K.PLAIN))
    cut_total = 0
    for combo in combos:
        mine = [docs for cls_id, sep_id, docs in batches if (cls_id, sep_id) == combo]
        assert [len(d) for d in mine] == [1, r - 1, r, r + 1, 3 * r + 2]
        room = max_len - sum(x is not None for x in combo)
        for docs in mine:
            ids, splits, _ = R.encode_rows(m, docs)
            lens = {splits[i + 1] - splits[i] for i in range(len(docs))}
            if len(docs) >= 5:
                assert lens == {0, max(0, room - 1), room, room + 1, 3 * max_len}, (max_len, combo, lens)
            else:
                assert lens <= {0, max(0, room - 1), room, room + 1, 3 * max_len}
            rows, lengths, cut = R.pack(ids, splits, max_len, combo[0], combo[1], K.PAD)
            assert cut == sum(1 for i in range(len(docs)) if splits[i + 1] - splits[i] > room)
            assert K.PAD not in ids and K.CLS not in ids and K.SEP not in ids
            cut_total += cut
    assert cut_total > 0


def test_lane_group_widths():
    assert {K.lanes_for(m) for m in K.MAX_LENS} == {4, 8, 16, 32, 64}
