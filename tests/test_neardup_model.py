"""CPU checks of tests/neardup_model.py, the executable form of the near-duplicate contract: literal values of every
function (so that the model cannot drift with the kernels), its vector forms against its scalar ones, its clusters
against a brute-force restatement, and that the signature estimates the Jaccard similarity."""
import math
import random

import numpy as np

import neardup_model as M
import wordpiece_amd as W


def test_literal_values_pin_the_functions():
    assert M.mix(0) == 0 and M.mix(1) == 0xb456bcfc34c2cb2c
    for shingle, plain, seeded in ((b"", 0xe5b9a9d7, 0xfb5273d6), (b"a", 0x24c6431a, 0xc203da9f), (b"abcde", 0x6ea81397, 0xd24b8445),
                                   (b"abcdefgh", 0x999a35a6, 0xb1b4f50a), (b"abcdefghi", 0x782bb7d2, 0xf97e4eee),
                                   (b"the quick brown fox", 0x650d1a2c, 0x5708889f)):
        assert M.shingle_x32(shingle) == plain and M.shingle_x32(shingle, seed=7) == seeded, shingle
    assert M.shingle_x32(np.array([5, 6], dtype=np.int32).tobytes()) == 0x9bea59c0  # two ids: one 64-bit word
    assert M.perm_ab(0) == (0x9ca066f1a4ab2eea, 0xd30b054265133dd7)
    assert M.perm_ab(3, seed=7) == (0x9e94d3dfd458dd83, 0x43d2f2434a681d15)
    a, b = M.perm_ab(0)
    assert M.perm(0, 0x6ea81397) == ((a * 0x6ea81397 + b) % 2 ** 64) >> 32 < 2 ** 32
    sig = M.signature(b"hello, world of shingles", 1, 5, 8)
    assert sig.dtype == np.uint32 and sig.tolist() == [0x13bba5e6, 0x17728cd7, 0x226664c3, 0xb66f650, 0x5491c5c, 0x4d1e94f, 0x709e908, 0x24829baa]
    assert M.band_key(sig, 1, 4) == 0xe0dab35960292c83 and M.band_key(sig, 0, 8, seed=7) == 0x649ad55e5bd38b53
    assert M.signature(b"", 1, 5, 3).tolist() == [0xffffffff] * 3
    assert M.lsh_min_agree(0.5, 128) == W.lsh_min_agree(0.5, 128) == 64 and W.lsh_min_agree(0.7, 128) == 90 and W.lsh_min_agree(0, 5) == 0


def test_mix_is_the_finaliser_of_the_kernels():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wordpiece_amd", "csrc", "group.h")).read()
    body = re.search(r"uint64_t mix64\(uint64_t h\) \{(.*?)\n\}", src, re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == ("h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; "
                                                  "h ^= h >> 33; return h;")


def test_vector_forms_equal_the_scalar_ones():
    row = bytes(range(40, 40 + 73))
    for eb, k in ((1, 1), (1, 2), (1, 5), (1, 8), (1, 9), (1, 16), (1, 64), (1, 100), (4, 1), (4, 2), (4, 3), (4, 5), (4, 64)):
        for seed in (0, 2 ** 63 + 5):
            r = row[:len(row) // eb * eb]
            n = len(r) // eb
            exp = [M.shingle_x32(r, seed)] if n < k else [M.shingle_x32(r[i * eb:(i + k) * eb], seed) for i in range(n - k + 1)]
            assert [int(x) for x in M.row_x32(r, eb, k, seed)] == exp, (eb, k)
            sig = M.signature(r, eb, k, 5, seed)
            assert [int(x) for x in sig] == [min(M.perm(j, x, seed) for x in exp) for j in range(5)], (eb, k)


def brute_force(rows, eb, k, n_perm, bands, min_agree, seed):
    """the contract restated without the model's bookkeeping: buckets by dict, edges to the smallest member, components by
    relabelling every edge's two rows to the smaller label until nothing changes"""
    r = n_perm // bands
    sigs = [M.signature(row, eb, k, n_perm, seed) for row in rows]
    buckets = {}
    for i, row in enumerate(rows):
        if row:
            for b in range(bands):
                buckets.setdefault(M.band_key(sigs[i], b, r, seed), set()).add(i)
    edges = set()
    for members in buckets.values():
        head = min(members)
        for m in members:
            if m != head and sum(1 for j in range(n_perm) if sigs[m][j] == sigs[head][j]) >= min_agree:
                edges.add((m, head))
    label = list(range(len(rows)))
    changed = True
    while changed:
        changed = False
        for m, h in edges:
            lo = min(label[m], label[h])
            if label[m] != lo or label[h] != lo:
                label[m] = label[h] = lo
                changed = True
    return label, edges


def test_clusters_equal_a_brute_force_restatement():
    rng = random.Random(11)
    words = [bytes(rng.randrange(97, 123) for _ in range(rng.randrange(1, 7))) for _ in range(30)]
    seen_joined = seen_split = False
    for trial in range(40):
        eb = rng.choice((1, 4))
        base = [b" ".join(rng.choice(words) for _ in range(rng.randrange(0, 12))) for _ in range(6)]
        rows = []
        for _ in range(rng.randrange(1, 25)):
            row = bytearray(rng.choice(base))
            for _ in range(rng.randrange(0, 3)):  # a typo or two
                if row:
                    row[rng.randrange(len(row))] = rng.randrange(97, 123)
            rows.append(bytes(row[:len(row) // eb * eb]))
        k, n_perm = rng.choice((1, 2, 5)), rng.choice((8, 16, 32))
        bands = rng.choice([b for b in (1, 2, 4, 8, 16, 32) if n_perm % b == 0])
        min_agree = rng.choice((0, n_perm // 4, n_perm // 2, n_perm))
        seed = rng.randrange(2 ** 64)
        data, off = M.join(rows, eb)
        got = M.neardup_rows(data, off, eb, k, n_perm, bands, min_agree, seed)
        label, edges = brute_force(rows, eb, k, n_perm, bands, min_agree, seed)
        assert got["cluster"] == label and got["edges"] == edges, trial
        assert got["kept"] == [i for i in range(len(rows)) if label[i] == i]
        assert got["counts"] == [label.count(i) for i in got["kept"]] and [got["kept"][s] for s in got["inverse"]] == label
        assert got["data"] == b"".join(rows[i] for i in got["kept"]) and got["row_off"][-1] * eb == len(got["data"])
        st = got["stats"]
        assert st["n_unique"] == len(got["kept"]) and st["n_empty"] == sum(1 for r in rows if not r) and st["n_candidates"] >= st["n_edges"] >= len(edges)
        seen_joined = seen_joined or len(got["kept"]) < len(rows)
        seen_split = seen_split or any(c > 1 for c in got["counts"]) and len(got["kept"]) > 1
    assert seen_joined and seen_split


def test_empty_rows_and_equal_rows():
    rows = [b"", b"abcdefgh", b"", b"abcdefgh", b"ab", b"ab", b""]
    got = M.neardup_rows(*M.join(rows), shingle=5, n_perm=16, bands=4, min_agree=16)
    assert got["cluster"] == [0, 1, 2, 1, 4, 4, 6]  # empty rows stay alone; equal rows join, shorter than a shingle too
    assert got["stats"]["n_shingles"] == 2 * 4 + 2 * 1 and got["stats"]["n_empty"] == 3
    assert (got["signatures"][0] == 0xffffffff).all() and (got["signatures"][1] == got["signatures"][3]).all()


def test_the_signature_estimates_the_jaccard_similarity():
    """Rows of 1,000 ids (k = 1), n_perm = 256, seed 0: agree / n_perm within 5 binomial deviations sqrt(J (1 - J) / n_perm)
    of J.  The run is deterministic; the z-values of the five overlaps J = 0.0526, 0.1998, 0.4286, 0.6667, 0.8182 are
    0.43, 1.07, 0.41, 0.31, -0.56 (agree = 15, 58, 113, 173, 206)."""
    n, n_perm = 1000, 256
    zs = []
    for shared in (100, 333, 600, 800, 900):
        a = np.arange(n, dtype=np.int32)
        b = np.concatenate([np.arange(shared, dtype=np.int32), np.arange(10 ** 6, 10 ** 6 + n - shared, dtype=np.int32)])
        J = shared / (2 * n - shared)
        agree = int((M.signature(a.tobytes(), 4, 1, n_perm) == M.signature(b.tobytes(), 4, 1, n_perm)).sum())
        z = (agree / n_perm - J) / math.sqrt(J * (1 - J) / n_perm)
        print("J %.4f agree %d z %.2f" % (J, agree, z))
        zs.append(z)
        assert abs(z) <= 5, (shared, z)
    assert max(abs(z) for z in zs) < 2.5  # (the room the seed was chosen for)
