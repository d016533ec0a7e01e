"""The model of the duplicate-row removal (tests/dedup_model.py) against numpy.unique and against cases worked by hand."""
import random

import numpy as np

import dedup_model as DM


def test_model_equals_numpy_unique_on_fixed_length_rows():
    rng = np.random.default_rng(3)
    for n, width, values in ((1, 1, 2), (50, 1, 3), (400, 3, 2), (1000, 2, 4), (300, 5, 2)):
        rows = rng.integers(0, values, size=(n, width), dtype=np.uint8)
        off = np.arange(n + 1) * width
        got = DM.dedup_rows(rows.tobytes(), off)
        _, idx, inv, cnt = np.unique(rows, axis=0, return_index=True, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        assert got["first"] == idx[inv].tolist()
        assert got["kept"] == sorted(idx.tolist())
        assert sorted(zip(got["kept"], got["counts"])) == sorted(zip(idx.tolist(), cnt.tolist()))
        fixed = DM.dedup_fixed(rows)
        for key in ("first", "kept", "counts", "inverse"):
            assert fixed[key].tolist() == got[key], key
        # int32 elements: the same rows, four bytes per element
        wide = rows.astype(np.int32) << 24
        got4 = DM.dedup_rows(wide.tobytes(), off, elem_bytes=4)
        assert (got4["first"], got4["kept"], got4["counts"], got4["inverse"]) == (got["first"], got["kept"], got["counts"], got["inverse"])
        assert got4["row_off"] == got["row_off"] and got4["stats"]["n_elems"] == n * width


def test_hand_cases():
    data, off = DM.join([b"ab", b"a", b"abc", b"ab", b"", b"a", b""])  # prefixes of each other, and empty rows
    r = DM.dedup_rows(data, off)
    assert r["first"] == [0, 1, 2, 0, 4, 1, 4] and r["kept"] == [0, 1, 2, 4] and r["counts"] == [2, 2, 1, 2]
    assert r["inverse"] == [0, 1, 2, 0, 3, 1, 3] and r["data"] == b"abaabc" and r["row_off"] == [0, 2, 3, 6, 6]
    assert r["stats"] == {"n_rows": 7, "n_unique": 4, "n_empty": 2, "n_elems": 9}
    r = DM.dedup_rows(*DM.join([b"xy"] * 5))  # all equal
    assert r["first"] == [0] * 5 and r["kept"] == [0] and r["counts"] == [5] and r["data"] == b"xy" and r["row_off"] == [0, 2]
    r = DM.dedup_rows(*DM.join([bytes([k]) for k in range(6)]))  # all distinct
    assert r["first"] == list(range(6)) == r["kept"] == r["inverse"] and r["counts"] == [1] * 6 and r["row_off"] == list(range(7))
    r = DM.dedup_rows(b"", [0, 0, 0])  # all empty
    assert r["first"] == [0, 0] and r["kept"] == [0] and r["counts"] == [2] and r["data"] == b"" and r["row_off"] == [0, 0]
    r = DM.dedup_rows(b"", [0])  # no row
    assert r["first"] == [] == r["kept"] == r["counts"] == r["inverse"] and r["row_off"] == [0]
    assert r["stats"] == {"n_rows": 0, "n_unique": 0, "n_empty": 0, "n_elems": 0}
    r = DM.dedup_rows(b"abcdefgh", [0, 2], want=0)  # bytes behind the last row are not read
    assert r["kept"] == [0] and "inverse" not in r and "data" not in r
    # ids: the same bytes at another element boundary are other rows
    ids = np.array([1, 2, 1, 2, 513], dtype=np.int32)
    r = DM.dedup_rows(ids.tobytes(), [0, 2, 4, 5], elem_bytes=4)
    assert r["first"] == [0, 0, 2] and r["row_off"] == [0, 2, 3] and np.frombuffer(r["data"], dtype=np.int32).tolist() == [1, 2, 513]


def test_identities_and_the_compact_form_is_a_fixed_point():
    rng = random.Random(9)
    for trial in range(30):
        pool = [bytes(rng.randrange(3) for _ in range(rng.randrange(0, 6))) for _ in range(rng.randrange(1, 12))]
        rows = [rng.choice(pool) for _ in range(rng.randrange(0, 60))]
        data, off = DM.join(rows)
        r = DM.dedup_rows(data, off)
        n = len(rows)
        assert sum(r["counts"]) == n and len(r["kept"]) == len(set(rows)) == r["stats"]["n_unique"]
        assert all(r["first"][i] == r["kept"][r["inverse"][i]] for i in range(n))
        assert all(r["first"][i] <= i and rows[r["first"][i]] == rows[i] for i in range(n))
        assert r["kept"] == sorted(r["kept"]) == [i for i in range(n) if r["first"][i] == i]
        again = DM.dedup_rows(r["data"], r["row_off"])
        u = len(r["kept"])
        assert again["first"] == list(range(u)) == again["kept"] == again["inverse"] and again["counts"] == [1] * u
        assert again["data"] == r["data"] and again["row_off"] == r["row_off"]
