"""CPU checks of the overlap contract's executable form (overlap_model.py) on cases small enough to work out by hand, and
of the constructed inputs of the GPU tests (overlap_cases.py): which positions hit, and that a case really puts a window
across a tile edge."""
import numpy as np
import pytest

import overlap_cases as K
import overlap_model as M


def run(rows, refs, eb=1, **kw):
    data, off = M.join(rows, eb)
    rdata, roff = M.join(refs, eb)
    return M.overlap_rows(data, off, rdata, roff, elem_bytes=eb, **kw)


def ids(*values):
    return np.array(values, dtype=np.int32).tobytes()


def test_k_1_is_element_membership():
    r = run([b"abca", b"", b"xyz"], [b"ca", b"z"], ngram=1)
    assert r["hits"] == [3, 0, 1] and r["first_hit"] == [0, -1, 2] and r["first_ref"] == [0, -1, 1] and r["covered"] == [3, 0, 1]
    assert r["mask"] == [1, 0, 1, 1, 0, 0, 1] and r["ref_hits"] == [2, 1] and r["kept"] == [1]
    assert r["stats"] == {"n_rows": 3, "n_ref": 2, "n_elems": 7, "n_ref_elems": 3, "n_windows": 7, "n_ref_windows": 3, "n_ref_distinct": 3,
                          "n_hits": 4, "n_hit_rows": 2, "n_covered": 4}


def test_a_window_across_two_rows_does_not_hit():
    r = run([b"abc", b"def"], [b"cd", b"bcde"], ngram=2)  # "cd" lies across the boundary
    assert r["hits"] == [1, 1] and r["first_hit"] == [1, 0] and r["first_ref"] == [1, 1] and r["mask"] == [0, 1, 1, 1, 1, 0]
    assert r["ref_hits"] == [0, 2]  # ("cd" of the second reference row is met by no corpus window)


def test_rows_of_k_minus_1_k_and_k_plus_1_elements():
    r = run([b"ab", b"abc", b"abcd"], [b"abc", b"bcd", b"ab"], ngram=3)
    assert r["hits"] == [0, 1, 2] and r["first_hit"] == [-1, 0, 0] and r["first_ref"] == [-1, 0, 0] and r["covered"] == [0, 3, 4]
    assert r["ref_hits"] == [1, 1, 0] and r["stats"]["n_windows"] == 3 and r["stats"]["n_ref_windows"] == 2
    r = run([ids(1, 2), ids(1, 2, 3), ids(1, 2, 3, 4)], [ids(9, 1, 2, 3)], eb=4, ngram=3)
    assert r["hits"] == [0, 1, 1] and r["first_hit"] == [-1, 0, 0] and r["covered"] == [0, 3, 3] and r["mask"] == [0, 0, 1, 1, 1, 1, 1, 1, 0]


def test_overlapping_hits_cover_a_union():
    r = run([b"xabcdey"], [b"abcde"], ngram=3)  # hits at 1, 2, 3: covered 5, not 9
    assert r["hits"] == [3] and r["first_hit"] == [1] and r["covered"] == [5] and r["mask"] == [0, 1, 1, 1, 1, 1, 0]
    r = run([b"abc__abc"], [b"abc"], ngram=3)  # two hits apart: 6
    assert r["hits"] == [2] and r["covered"] == [6] and r["ref_hits"] == [1]  # (the reference window is counted once)


def test_the_smaller_reference_row_wins():
    refs = [b"q"] * 3 + [b"hello"] + [b"q"] * 3 + [b"ahellob"]
    r = run([b"say hello"], refs, ngram=5)
    assert r["hits"] == [1] and r["first_hit"] == [4] and r["first_ref"] == [3] and r["ref_hits"] == [0, 0, 0, 1, 0, 0, 0, 1]


def test_a_reference_row_of_one_repeated_element():
    r = run([b"zaaaaz", b"aaa"], [b"a" * 50], ngram=3)
    assert r["stats"]["n_ref_distinct"] == 1 and r["stats"]["n_ref_windows"] == 48
    assert r["hits"] == [2, 1] and r["covered"] == [4, 3] and r["ref_hits"] == [48]


def test_text_rows_that_start_at_odd_bytes():
    r = run([b"a", b"bcd", b"", b"efghi"], [b"x", b"cd", b"ghi"], ngram=2)
    assert r["hits"] == [0, 1, 0, 2] and r["first_hit"] == [-1, 1, -1, 2] and r["first_ref"] == [-1, 1, -1, 2] and r["covered"] == [0, 2, 0, 3]


def test_max_hits_0_and_1():
    rows, refs = [b"abab", b"abxx", b"xxxx"], [b"ab"]
    r = run(rows, refs, ngram=2, max_hits=0)
    assert r["hits"] == [2, 1, 0] and r["kept"] == [2] and r["data"] == b"xxxx" and r["row_off"] == [0, 4]
    r = run(rows, refs, ngram=2, max_hits=1)
    assert r["kept"] == [1, 2] and r["data"] == b"abxxxxxx" and r["row_off"] == [0, 4, 8]
    r = run(rows, refs, ngram=2, want=0)
    assert "kept" not in r and "mask" not in r and "ref_hits" not in r


def test_an_empty_reference_set_and_no_rows():
    for refs in ([], [b""], [b"ab"]):
        r = run([b"abc", b""], refs, ngram=3)
        assert r["hits"] == [0, 0] and r["first_hit"] == [-1, -1] and r["first_ref"] == [-1, -1] and r["covered"] == [0, 0] and r["kept"] == [0, 1]
        assert r["mask"] == [0, 0, 0] and r["ref_hits"] == [0] * len(refs) and r["data"] == b"abc" and r["row_off"] == [0, 3, 3]
    r = run([], [b"abc"], ngram=2)
    assert r["hits"] == [] and r["kept"] == [] and r["row_off"] == [0] and r["stats"]["n_ref_distinct"] == 2 and r["stats"]["n_elems"] == 0


# ---- the constructed inputs of test_gpu_overlap.py ----------------------------------------------------------------------

def test_the_tile_constant_leaves_room_for_the_halo():
    T = K.tile()
    assert T >= 256 and T % 64 == 0


@pytest.mark.parametrize("eb,k", [(4, 1), (4, 2), (4, 13), (4, 64), (1, 13), (1, 63)])
def test_tile_edge_case_hits_exactly_the_planted_positions(eb, k):
    T = K.tile()
    rows, refs, eb, facts = K.tile_edge_case(T, k, eb)
    r = run(rows, refs, eb=eb, ngram=k)
    planted = facts["planted"]
    assert facts["n"] == 3 * T + 5 and planted[-1] == facts["n"] - k and T - k in planted and T + 1 in planted
    assert any(p < T < p + k for p in planted) or k == 1  # a planted window lies across the tile edge
    assert any(p + k == T for p in planted)               # ... and one ends exactly at it
    hit = [p for p in range(facts["n"] - k + 1) if rows[0][p * eb:(p + k) * eb] in set(refs)]
    assert hit == planted and r["hits"] == [len(planted)] and r["first_hit"] == [planted[0]]
    assert r["covered"] == [len(set(e for p in planted for e in range(p, p + k)))]


@pytest.mark.parametrize("eb", [1, 4])
@pytest.mark.parametrize("shift", [-1, 0, 1])
def test_boundary_case_straddles_and_does_not_hit(eb, shift):
    T = K.tile()
    rows, refs, eb, facts = K.boundary_case(T, 13, eb, T + shift)
    s = facts["straddle"]
    assert s < T + shift < s + 13 and facts["flat"][s * eb:(s + 13) * eb] == refs[0]  # the bytes across the boundary are the reference window
    r = run(rows, refs, eb=eb, ngram=13)
    assert r["hits"] == [0, 0] and r["ref_hits"] == [0] and r["stats"]["n_ref_windows"] == 1
    joined = run([b"".join(rows)], refs, eb=eb, ngram=13)  # without the boundary it would hit
    assert joined["hits"] == [1] and joined["first_hit"] == [s]


def test_unit_rows_and_long_row_cases():
    T = K.tile()
    rows, refs, eb, facts = K.unit_rows_case(T, 5, 4)
    r = run(rows, refs, eb=eb, ngram=5)
    assert len(rows) == T and [i for i, h in enumerate(r["hits"]) if h] == facts["hit_rows"] and max(r["hits"]) == 1
    rows, refs, eb, facts = K.long_row_case(long_n=30_000)
    r = run(rows, refs, eb=eb, ngram=13)
    long = facts["long"]
    assert r["hits"][long] == facts["hits"] and r["covered"][long] == facts["covered"] < 13 * facts["hits"] and sum(r["hits"]) == facts["hits"]
    assert 0.2 < facts["hits"] / (30_000 - 12) < 0.3 and r["first_hit"][long] == 0 and r["ref_hits"] == [100] * len(refs)
