"""CPU checks of tests/repeat_model.py, the executable form of the repeated-span contract: against a quadratic brute force
on random batches, on cases pinned by hand, and on the constructed cases of repeat_cases.py, whose promises
test_gpu_repeat.py relies on."""
import numpy as np
import pytest

import repeat_cases as K
import repeat_model as M


def run(rows, eb=1, **spec):
    data, off = M.join(rows, eb)
    return M.repeat_rows(data, off, elem_bytes=eb, **spec)


def test_model_equals_the_brute_force_on_random_batches():
    rng = np.random.default_rng(1)
    for it in range(300):
        eb = 1 if it % 2 else 4
        k = (1, 2, 3, 5)[it % 4]
        scope = (it // 4) % 2
        alphabet = int(rng.integers(2, 5))
        rows = [K.elems(rng.integers(0, alphabet, int(n)), eb) for n in rng.integers(0, 14, int(rng.integers(1, 7)))]
        data, off = M.join(rows, eb)
        got = M.repeat_rows(data, off, elem_bytes=eb, ngram=k, scope=scope)
        repeats, src, mask = M.brute_force(data, off, elem_bytes=eb, ngram=k, scope=scope)
        assert (got["repeats"], got["src"], got["mask"]) == (repeats, src, mask), (it, rows, k, scope)
        assert got["covered"] == [sum(mask[off[i]:off[i + 1]]) for i in range(len(rows))]
        for i in range(len(rows)):
            hits = [p for p in range(off[i + 1] - off[i]) if src[off[i] + p] >= 0]
            assert got["first_repeat"][i] == (hits[0] if hits else -1)
            if hits:
                at = src[off[i] + hits[0]]
                r = got["first_src_row"][i]
                assert off[r] <= at < off[r + 1] and got["first_src_pos"][i] == at - off[r]
            else:
                assert (got["first_src_row"][i], got["first_src_pos"][i]) == (-1, -1)
        if scope == 0:
            assert got["stats"]["n_repeats"] == got["stats"]["n_windows"] - got["stats"]["n_distinct"]


def test_pinned_cases():
    r = run([b"aaaaa"], ngram=2)  # windows at 0..3, all "aa": 1..3 repeat position 0; element 0 lies in no repeat window
    assert (r["repeats"], r["first_repeat"], r["first_src_row"], r["first_src_pos"], r["covered"]) == ([3], [1], [0], [0], [4])
    assert r["src"] == [-1, 0, 0, 0, -1] and r["mask"] == [0, 1, 1, 1, 1] and r["cut_data"] == b"a"
    assert run([b"aaaa"], ngram=2)["cut_data"] == b"a"  # the first occurrence is no repeat, but other windows cover its second element
    r = run([b"abababab"], ngram=3)  # period 2: every p >= 2 repeats p mod 2
    assert r["src"] == [-1, -1, 0, 1, 0, 1, -1, -1] and r["repeats"] == [4] and r["covered"] == [6]
    # a row equal to an earlier one: both scopes agree
    for scope in (0, 1):
        r = run([b"hello world", b"xyz", b"hello world"], ngram=4, scope=scope)
        assert r["repeats"] == [0, 0, 8] and r["covered"] == [0, 0, 11] and r["first_src_row"] == [-1, -1, 0] and r["cut_off"] == [0, 11, 14, 14]
        assert r["kept"] == [0, 1] and r["data"] == b"hello worldxyz" and r["row_off"] == [0, 11, 14]
    # a row that only repeats itself: scope 1 finds nothing
    assert run([b"q", b"abcabcabc"], ngram=3, scope=0)["repeats"] == [0, 4]
    r = run([b"q", b"abcabcabc"], ngram=3, scope=1)
    assert r["repeats"] == [0, 0] and r["covered"] == [0, 0] and r["cut_data"] == b"qabcabcabc" and r["stats"]["n_repeats"] == 0
    # scope 1 keeps what the row repeats of itself and still finds what it repeats of earlier rows
    r = run([b"abcd", b"xyxyxy abcd"], ngram=4, scope=1)
    assert r["repeats"] == [0, 1] and r["first_repeat"] == [-1, 7] and r["first_src_pos"] == [-1, 0] and r["covered"] == [0, 4]
    # piecewise cover from two sources: "abcd" from row 0 and "cdef" from row 1 cover "abcdef"
    r = run([b"abcd", b"cdef", b"abcdef"], ngram=4)
    assert r["repeats"] == [0, 0, 2] and r["src"][8:] == [0, -1, 4, -1, -1, -1] and r["covered"] == [0, 0, 6] and r["cut_off"] == [0, 4, 8, 8]


def test_the_cut_is_the_data_without_the_mask():
    rng = np.random.default_rng(2)
    for it in range(60):
        eb = 1 if it % 2 else 4
        rows = [K.elems(rng.integers(0, 3, int(n)), eb) for n in rng.integers(0, 30, 6)]
        data, off = M.join(rows, eb)
        r = M.repeat_rows(data, off, elem_bytes=eb, ngram=int(rng.integers(1, 6)), scope=it // 2 % 2)
        flat = np.frombuffer(data, dtype=np.uint8 if eb == 1 else np.int32)
        mask = np.array(r["mask"], dtype=np.uint8)
        assert flat[mask == 0].tobytes() == r["cut_data"]
        assert r["cut_off"] == [0] + list(np.cumsum([l - c for l, c in zip(np.diff(off), r["covered"])]))
        assert r["stats"]["n_cut_elems"] == r["cut_off"][-1] == len(flat) - r["stats"]["n_covered"]
        assert M.repeat_rows(data, off, elem_bytes=eb, want=7)["stats"]["n_cut_elems"] == 0


def test_utf8_windows_keep_the_cut_decodable():
    docs, text = K.utf8_pair()
    rows = [d.encode("utf8") for d in docs]
    k = len(text) + 1  # a window that begins on the shared A9
    assert rows[0][1:] == rows[1][1:] and rows[0][1] == 0xa9 and rows[0][0] != rows[1][0]
    raw = run(rows, ngram=k)
    assert raw["repeats"] == [0, 1] and raw["first_repeat"] == [-1, 1] and raw["cut_data"][len(rows[0]):] == rows[1][:1]
    with pytest.raises(UnicodeDecodeError):  # without the flag the cut leaves the lead byte of the e with acute alone
        raw["cut_data"].decode("utf8")
    r = run(rows, ngram=k, utf8=True)
    assert r["repeats"] == [0, 0] and r["cut_data"].decode("utf8") == "".join(docs)
    r = run(rows, ngram=len(text), utf8=True)  # the text behind the sign: a window at a code point boundary
    assert r["repeats"] == [0, 1] and r["first_repeat"] == [-1, 2] and r["cut_data"].decode("utf8") == docs[0] + "é"
    # a window may not end inside a sequence either, and ineligible positions are no sources
    r = run(["xab©".encode("utf8"), "ab©".encode("utf8")], ngram=3, utf8=True)
    assert r["repeats"] == [0, 1] and r["first_repeat"] == [-1, 1] and r["stats"]["n_windows"] == 2 + 1  # ("xab", "b©" | "b©": "ab\xc2" ends inside the sign)
    r = run(["xab©".encode("utf8"), "ab©".encode("utf8")], ngram=3)
    assert r["repeats"] == [0, 2]
    with pytest.raises(AssertionError):
        run([np.arange(4, dtype=np.int32).tobytes()], eb=4, ngram=2, utf8=True)
    # invalid text: the rule reads bytes only
    r = run([b"\x80\x80ab\x80", b"\x80ab"], ngram=2, utf8=True)
    assert r["stats"]["n_windows"] == 1 + 1 and r["repeats"] == [0, 0]  # ("b\x80" at the end of row 0, "ab" at the end of row 1: the "ab" of row 0 ends in front of a continuation byte)


T = K.tiles()


def test_constructed_cases_keep_their_promises():
    assert T["T"] + T["halo"] <= 1280 and T["tile"] % 4 == 0 and T["cut"] % 4 == 0
    for tile in (T["T"], T["tile"]):
        for k in (1, 2, 13, 63, 64):
            pairs = K.edge_starts(tile, k)
            assert {s for s, _ in pairs} == {3 * tile - k, 3 * tile - 1, 3 * tile} and len({s // tile - q // tile for s, q in pairs}) == 3
            for eb in (1, 4):
                if eb == 1 and k < 4:
                    continue  # (short text windows repeat by themselves; the device is held against the model all the same)
                for start, src in pairs[::3]:
                    rows, _, _ = K.edge_case(tile, k, eb, start, src)
                    r = run(rows, eb, ngram=k)
                    assert r["src"][start] == src  # (in text the element behind the copy may happen to go on like the one behind the source)
                    assert eb == 1 or (r["repeats"], r["first_repeat"], r["first_src_pos"], r["covered"]) == ([1], [start], [src], [k])
    for eb in (1, 4):
        rows, _, facts = K.row_end_case(T["T"], 13, eb, T["T"] + 1)
        assert run(rows, eb, ngram=13)["repeats"] == facts["repeats"]
        rows, _, facts = K.unit_rows_case(64, 5, eb)
        r = run(rows, eb, ngram=5)
        assert [i for i, x in enumerate(r["repeats"]) if x] == facts["repeat_rows"] and r["stats"]["n_distinct"] == 32
        rows, _, facts = K.sized_case(2 * T["T"], 13, eb)
        assert sum(len(x) for x in rows) == 2 * T["T"] * eb and sum(run(rows, eb, ngram=13)["repeats"]) > 300
    rows, _, _ = K.periodic_case(300)
    r = run(rows, ngram=13)
    assert r["src"][:300 - 12] == [-1, -1] + [p % 2 for p in range(2, 300 - 12)] and r["covered"] == [298]
    for eb in (1, 4):
        rows, _, _ = K.multiplicity_case(7, eb)
        r = run(rows, eb, ngram=7)
        assert r["repeats"] == [0, 0, 999, 5, 5, 0, 1] and r["first_src_row"] == [-1, -1, 2, 1, 1, -1, 1] and r["stats"]["n_distinct"] == r["stats"]["n_windows"] - 1010
        rows, _, facts = K.cut_case(6, eb, T["cut"])
        r = run(rows, eb, ngram=6)
        cut_rows = np.diff(r["cut_off"]).tolist()
        assert all(cut_rows[i] == 0 for i in facts["empty"]) and cut_rows[1] == 5 and cut_rows[3] == 3
        m, c = r["mask"], T["cut"]
        assert m[c - 2:c + 2] == [0] * 4 and m[2 * c - 2:2 * c + 2] == [1] * 4 and len(m) > 2 * c
        starts = {sum(1 for x in m[:e] if not x) % 4 for e in range(1, len(m)) if m[e - 1] and not m[e]}
        assert eb == 4 or starts == {0, 1, 2, 3}  # kept runs of bytes begin at every alignment of the output
