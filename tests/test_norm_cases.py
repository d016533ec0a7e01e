"""CPU tests of the inputs behind test_gpu_norm_edges.py (norm_cases.py): the layout constants are the headers'; the layout
model is right on texts small enough to check by eye; and it reproduces what every builder claims to have built: the path
every chunk takes (A, M), every kept ASCII value at each of the 16 positions of a chunk of that path and the named
neighbours (A), what a row gives and at which alignment (X), what a tile gives (X), the lead s bytes in front of the named
boundary and what stands there (S), one id per non-blank normalised code point under single_symbol_vocab (M), and the
shapes of the sequences (H).  T's tables over the whole code space are not built here: the text's size and order are."""
import collections

import pytest

import norm_cases as N
import normalize_model as NM
import offsets_model as OM
from bruteforce import is_space
from test_normalize_tables import _same_unicode


def test_constants_are_read_from_the_headers():
    assert (N.CHUNK, N.LANES, N.ROW, N.WAVE, N.TILE, N.ROW_OUT) == (16, 64, 1024, 4096, 16384, 3084), \
        "a constant of the layout changed: the cases moved with it — check GROUP_SIZES and update this line"
    assert N.ROW_OUT == 3 * (N.ROW + 4) and N.ROWS_PER_TILE == 16
    assert {k: N.boundary_kind(x) for k, x in N.S_BOUNDARIES.items()} == {k: k for k in N.S_BOUNDARIES}


def test_case_count_per_group():
    count = collections.Counter(n[0] for n in N.CASES)
    assert dict(count) == N.GROUP_SIZES
    for n in N.X_GIVES:
        for a in range(4):
            assert {"X_gives%d_a%d_%s" % (n, a, p) for p in ("wave", "tile", "ragged")} <= set(N.CASES)
    for kind in N.S_BOUNDARIES:
        for s in (1, 2, 3):
            assert sum(1 for n in N.CASES if n.startswith("S_%s_s%d_" % (kind, s))) == 3 * len(N.S_CPS) + len(N.S_INVALID)
    for name in N.CASES:
        assert len(N.build(name)[0]) <= N.MAX_TEXT


def test_layout_model_on_hand_made_texts():
    _same_unicode()
    m = N.Layout("Ab\u0001É각".encode(), 7)
    assert (m.norm, m.src_byte, m.src_cp) == ("abe각".encode(), [0, 1, 3, 5, 5, 5], [0, 1, 3, 4, 4, 4])
    assert m.rows == [dict(base=0, paths=["rule"] + [None] * 63, nb=12, nc=6, sc=5, out=0, a=0)] and m.tiles == [(12, 6, 5)]
    assert N.Layout("Ab\u0001É각".encode(), 6).rows[0]["paths"][0] == "lean"   # nothing dropped without WP_NORM_CLEAN
    # a full row of clean ASCII is a "row"; one byte short, its last lane is lean and the others are "lane"
    assert N.Layout(b"x" * N.ROW, 7).rows[0]["paths"] == ["row"] * 64
    assert N.Layout(b"x" * (N.ROW - 1), 7).rows[0]["paths"] == ["lane"] * 63 + ["lean"]
    m = N.Layout(b"x" * 16 + b"y\x7f" + b"z" * 14 + "é".encode() + b"w" * (2 * N.ROW - 34), 3)
    assert m.rows[0]["paths"] == ["lane", "rule", "lean"] + ["lane"] * 61 and m.rows[1]["paths"] == ["row"] * 64
    assert [(r["nb"], r["nc"], r["sc"], r["out"], r["a"]) for r in m.rows] == [(N.ROW - 1, N.ROW - 2, N.ROW - 1, 0, 0), (N.ROW, N.ROW, N.ROW, N.ROW - 1, 3)]
    assert N.Layout(m.text, 2).rows[0]["paths"] == ["lane", "lane", "lean"] + ["lane"] * 61
    # a code point belongs to the row that holds its lead
    m = N.Layout(b"x" * (N.ROW - 1) + "각".encode() + b"y" * 5, 4)
    assert [(r["nb"], r["nc"], r["sc"]) for r in m.rows] == [(N.ROW - 1 + 9, N.ROW - 1 + 3, N.ROW), (5, 5, 5)]
    assert m.path_at(N.ROW - 1) == "lean" and m.source_of_output_byte(N.ROW - 1 + 8) == N.ROW - 1 and m.source_of_output_byte(N.ROW + 8) == N.ROW + 2
    assert N.single_symbol_vocab("Ab É\u0001", 7) == ["[UNK]", "a", "b", "e", "##a", "##b", "##e"]


def _full_rows(m):
    return [r for r in m.rows if r["base"] + N.ROW <= m.nbytes]


def _chunks_of(m, path):
    for r in _full_rows(m):
        for lane, p in enumerate(r["paths"]):
            if p == path:
                yield m.text[r["base"] + lane * N.CHUNK:r["base"] + (lane + 1) * N.CHUNK]


def check_claims(name, text, expect):
    claims = dict(expect["claims"])
    assert claims, "every case states what it is"
    layouts = {}

    def lay(f):
        if f not in layouts:
            layouts[f] = N.Layout(text, f)
        return layouts[f]

    if "nbytes" in claims:
        assert len(text) == claims.pop("nbytes"), len(text)
    lane = claims.pop("lane", None)
    paths = claims.pop("paths", {})
    for f, path in paths.items():
        full = _full_rows(lay(f))
        assert len(full) >= max(2, claims.get("rows", 2))
        for r in full:
            want = [path] * N.LANES
            if lane is not None:
                want[lane] = "lean"
            assert r["paths"] == want, (f, r["base"], r["paths"])
    if name[0] in "AM":
        claims.pop("rows", None)
    every = claims.pop("covers_all_values", False)
    neighbours = claims.pop("neighbours", ())
    for f in claims.pop("covers", ()):
        values = range(128) if every else N.KEPT[f]
        seen = {(b, p) for chunk in _chunks_of(lay(f), paths[f]) for p, b in enumerate(chunk)}
        missing = [(v, p) for v in values for p in range(N.CHUNK) if (v, p) not in seen]
        assert not missing, (f, len(missing), missing[:5])
        assert all(n in values and (n, 0) in seen for n in neighbours if every or n in N.KEPT[f]), f
        assert {0x09, 0x0A, 0x0D, 0x20, 0x40, 0x41, 0x5A, 0x5B, 0x60, 0x61, 0x7A, 0x7B, 0x7E} <= set(values) & set(neighbours)
    for f, rows in claims.pop("rows", {}).items():
        for r, (nb, a) in rows.items():
            assert (lay(f).rows[r]["nb"], lay(f).rows[r]["a"]) == (nb, a), (f, r, lay(f).rows[r]["nb"], lay(f).rows[r]["a"])
        if "max_row" in claims:
            assert lay(f).rows[2]["nb"] == claims["max_row"] <= N.ROW_OUT and max(r["nb"] for r in lay(f).rows) == claims["max_row"]
    claims.pop("max_row", None)
    for f, rows in claims.pop("row_paths", {}).items():
        for r, path in rows.items():
            assert lay(f).rows[r]["paths"] == [path] * N.LANES, (f, r)
    for f, tiles in claims.pop("tiles", {}).items():
        for t, (nb, nc) in tiles.items():
            assert lay(f).tiles[t][:2] == (nb, nc) and lay(f).tiles[t][2] > 0, (f, t, lay(f).tiles[t])
    for f, tiles in claims.pop("tiles_give", {}).items():
        assert all(lay(f).tiles[t][0] > 0 for t in tiles), (f, lay(f).tiles)
    for f, n in claims.pop("norm_len", {}).items():
        assert len(lay(f).norm) == n, (f, len(lay(f).norm))
    if "seam" in claims:
        kind, X, pos = claims.pop("seam")
        starts = lay(0).starts
        assert N.boundary_kind(X) == kind and X - pos in (1, 2, 3) and text[pos] >= 0xC0 and text[pos - 1] < 0x80
        if "cp" in claims:
            cp = claims.pop("cp")
            seq = chr(cp).encode()
            assert pos in starts and lay(0).cps[starts.index(pos)] == cp
            for f, n in claims.pop("gives").items():
                assert len("".join(map(chr, NM.normalize_cp(f, cp))).encode()) == n, (f, n)
            follow = claims.pop("follow")
            assert text[pos + len(seq):pos + len(seq) + 1] == follow and (follow == b"Q" or not NM.normalize_cp(1, follow[0]))
        elif claims.pop("cut", False):
            assert (not starts or starts[-1] < pos) and OM.seq_len(text[pos]) == len(text) - pos + 1
        else:
            n = claims.pop("invalid")
            assert not any(pos <= s < pos + n for s in starts) and pos + n in starts and text[pos + n] == 0x51
    if "probe" in claims:
        at, row = claims.pop("probe")
        assert at // N.ROW == row and text[at:at + len(N.M_PROBE)] == N.M_PROBE
        for f in claims.pop("sums_differ"):
            sums = [sum(r[k] for r in lay(f).rows[:row]) for k in ("nb", "nc", "sc")]
            assert len(set(sums)) == 3, (f, sums)
            bases = [sum(t[k] for t in lay(f).tiles[:row // N.ROWS_PER_TILE]) for k in range(3)]
            assert bases[0] != bases[1] and bases[0] != bases[2], (f, bases)
    if claims.pop("one_id_per_cp", False):
        for f in N.MAP_FLAGS:
            vocab = N.single_symbol_vocab(text, f)
            ids, spans, t, _ = OM.encode_spans(N.model(text, f)[0], vocab)
            kept = [i for i, c in enumerate(t) if not is_space(c)]
            assert spans == [(i, i + 1) for i in kept] and 0 not in ids, (f, len(ids), len(kept))
    if "last_cp_bytes" in claims:
        assert len(chr(lay(0).cps[-1]).encode()) == claims.pop("last_cp_bytes")
    if "dropped_under_clean" in claims:
        assert len(lay(0).cps) - len(lay(1).src_cp) == claims.pop("dropped_under_clean")
    if claims.pop("split_syllable", False):
        ids, spans = NM.encode_spans_normalized(text, claims.pop("vocab"), 4, "char")
        k = ids.index(1)
        assert ids[k:k + 3] == [1, 2, 3] and spans[k] == spans[k + 1] == spans[k + 2] and spans[k][1] - spans[k][0] == 1
    if claims.pop("ends_in_expansion", False):
        assert lay(7).src_cp[-1] == lay(7).src_cp[-3] and lay(4).src_cp[-1] == lay(4).src_cp[-3]
    if claims.pop("composed", False):
        assert N.build(name)[0] == text
    assert not claims, claims


@pytest.mark.parametrize("name", N.names("AM"))
def test_case_is_what_its_builder_claims(name):
    _same_unicode()
    text, expect = N.build(name)
    check_claims(name, text, expect)


BLOCKS = 8


@pytest.mark.parametrize("block", range(BLOCKS))
def test_row_seam_and_composed_cases_are_what_their_builders_claim(block):
    """groups X, S and F, a block of names per test"""
    _same_unicode()
    for name in N.names("XSF")[block::BLOCKS]:
        text, expect = N.build(name)
        try:
            check_claims(name, text, expect)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))


def test_composed_cases_reach_every_path_and_alignment():
    """F: the 100 compositions together take every path, flush rows of 0..8 bytes and of more than a row at every alignment"""
    _same_unicode()
    paths, small, large = set(), set(), set()
    for name in N.names("F"):
        m = N.Layout(N.build(name)[0], 7)
        for r in m.rows:
            paths |= set(r["paths"])
            if r["nb"] <= 8:
                small.add((r["nb"] > 0, r["a"]))
            if r["nb"] > N.ROW:
                large.add(r["a"])
    assert paths == {"row", "lane", "lean", "rule", None} and small == {(x, a) for x in (False, True) for a in range(4)} and large == {0, 1, 2, 3}


def test_whole_code_space_text():
    """T: every scalar value once, in order, behind 0..3 ASCII bytes (the tables of what they give: test_gpu_norm_edges.py)"""
    text = N.t_text(3)
    assert len(text) == N.T_BYTES + 3 == 4382592 + 3
    cps, starts = OM.decode_with_starts(text[:70000])
    assert cps[:3] == [0x78] * 3 and cps[3:3 + 0x800] == list(range(0x800)) and starts[3 + 0x80] == 3 + 0x80
    assert text[3:] == N.t_text(0) and text.decode("utf8")[-1] == "\U0010ffff" and "\ud7ff\ue000".encode() in text
    sample = [chr(c).encode() for c in range(0x300)]
    good = b"xx" + b"".join(sample)
    assert N.t_first_difference(good, sample, 2) is None
    assert N.t_first_difference(good[:0x102] + b"e" + good[0x104:], sample, 2).startswith("U+00C0")
    assert N.t_first_difference(good + b"z", sample, 2) == "1 bytes behind the last code point"


def test_sequences():
    """H: the texts are what the sequences need"""
    first, second = N._h_long_then_lead()
    assert len(second) < len(first) and second[-1] >= 0xC0 and all(b & 0xC0 == 0x80 for b in first[len(second):len(second) + 2])
    assert first[:len(second) - 1] == second[:-1] and len(N.model(second, 7)[0]) == len(second) - 1
    for name, make in N.SEQUENCES.items():
        steps = make()
        assert len(steps) >= 3 and all(call in ("normalize", "encode", "offsets") and 0 <= f < 8 and text for call, text, f in steps), name
    assert [f for _, _, f in N.SEQUENCES["H_flags_7_2_0_7"]()][::2] == [7, 2, 0, 7]
    sizes = [len(N.model(t, f)[0]) for _, t, f in N.SEQUENCES["H_grow_between_calls"]()][::2]
    assert sizes[0] < sizes[1] > sizes[2] and sizes[0] < len(N.SEQUENCES["H_grow_between_calls"]()[0][1])   # shrinks, then expands
    # the shard rule: the middle of the text lies in front of U+000B, and behind it the first blank that
    # WP_NORM_CLEAN keeps is the one near the end
    text, k = N.shard_text(), N.H_SHARD_K
    mid = len(text) // 2
    assert mid < k and text[k:k + 2] == b"\x0b\x0c" and text[mid:k] == b"x" * (k - mid)
    blanks = [i for i in range(mid, len(text)) if is_space(text[i])]
    assert blanks == [k, k + 1, len(text) - 2]
    assert N.model(text, 1)[0] == b"x" * k + b"y" * (k - 16) + b" z" and N.model(text, 4)[0] == text
