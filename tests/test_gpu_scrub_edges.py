"""The scrub past its first tile and its first grid (csrc/scrub.h: scrub_find_kernel, scrub_docs_kernel, scrub_write_kernel;
scrub_path.h with the scans and the kept rows of text_path.h), on the batches of scrub_edge_cases.py: row counts at the wave,
workgroup and scan-tile edges, more row starts in a span than a workgroup has lanes, row starts on tile starts, data of one
byte to a byte past two tiles, addresses inside the domain and the local part of an e-mail, match lists at the scan tile, a
tile with as many matches as the write kernel stages, and seeded random rows of near-misses.  Every comparison is exact and
goes through test_gpu_scrub.check: every array and dtype of both forms and the statistics against tests/scrub_model.py.

Without a GPU: the geometry the cases are built from against the sources, every case's claim on the model's answer, and the
floors of the random batches (a random test that finds nothing proves nothing).

Wall time on an MI355X: 3.3 s for the 201 tests of this file (the model's share on the CPU: 0.6 s for all cases).  Found by this
file: nothing; every comparison held on the kernels as they were.  Wrong kernels that only this file notices (the older
test_gpu_scrub.py passes on each): the backward branch of sc_inside_email answering false (inside e-mails, random *); the grid
of scrub_docs_kernel one lane short at n_rows = 256 and 2048 (rows 256 *, rows 2048 *); the row-boundary loop of
scrub_find_kernel without its second step (tiny rows over a tile start, rows 2047 / 2048 / 2049 *, dense tile *)."""
import functools
import os
import subprocess
import sys

import pytest

import scrub_edge_cases as E
import scrub_model as M
from test_gpu_scrub import HERE, PKG, S, check, handle  # noqa: F401  (handle: the child of the hardened runs)


def test_geometry_the_cases_are_built_from():
    """a change of the tile, the halo or the scan tile fails here instead of moving the edges away from the cases"""
    src = E.geometry()
    assert src == {name: text for names in E.SOURCE.values() for name, text in names.items()}, src
    assert (E.WAVE, E.BLOCK, E.ITEMS) == (int(src["kWave"]), int(src["kBlock"]), int(src["kQualItems"])) and E.T == E.BLOCK * E.ITEMS == 2048
    assert E.FRONT == int(src["kScFront"]) and E.BEHIND == int(src["kScBehind"]) and E.TILE_MATCHES == E.T // 6 + 2 == 343
    assert E.SCAN_TILE == E.BLOCK * int(src["kScanItems"]) == 2048
    # the halo holds what the cases lean on: an '@' 256 bytes in front of an address with its local run and the byte in front of
    # that; behind an address the rest of a local run of 64 that began with it, the '@', and the 256 bytes that show a domain too long
    assert E.FRONT >= 256 + 65 and E.BEHIND >= 64 + 1 + 256
    assert E.ROW_COUNTS == (1, 63, 64, 255, 256, 257, 2047, 2048, 2049) and E.SIZES == (1, 5, 6, 2047, 2048, 2049, 4096, 4097)


@functools.lru_cache(maxsize=None)
def model(name):
    rows, how, _ = E.CASES[name]
    kinds = sum(1 << ("email", "ipv4").index(k) for k in how.get("kinds", ("email", "ipv4"))) | (M.KEEP_PRIVATE if how.get("keep_private") else 0)
    default = {k: [x.encode() for x in strings] for k, strings in S.scrub_replacements("default").items()}
    return M.scrub_rows(b"".join(rows), E.offsets(rows), kinds, how.get("email", default["email"]), how.get("ip", default["ip"]), how.get("rules"))


@pytest.mark.parametrize("name", sorted(n for n, c in E.CASES.items() if c[2]))
def test_every_case_is_what_its_name_says(name):
    rows, _, claim = E.CASES[name]
    claim(model(name), E.offsets(rows))


@pytest.mark.parametrize("seed", E.SEEDS)
def test_random_batches_meet_their_floors(seed):
    """on the model alone: the seeded rows hold enough of everything the differential test is about"""
    n = E.random_floors(E.CASES["random %d private" % seed][0])
    print(n)
    assert 300 <= n["rows"] <= 2000 and 3 * E.T <= n["bytes"] <= 8 * E.T, n
    assert all(n[k] >= floor for k, floor in E.FLOORS.items()), (n, E.FLOORS)
    lens = [len(x) for how in (E.RANDOM_HOW, E.LISTS) for k in ("email", "ip") for x in how[k]]
    assert 0 in lens and 64 in lens and E.FLOORS == dict(emails=20, replaced=20, private=3, suppressed=3, crossing=1, behind_tile_start=1)


def run(name):
    rows, how, claim = E.CASES[name]
    exp = check(rows, how, name)
    if claim:
        claim(exp, E.offsets(rows))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(E.CASES))
def test_edge_batches_against_the_model(name):
    run(name)


@pytest.mark.gpu
def test_a_smaller_batch_behind_a_larger_one():
    """the entry behind the last row and the list ends of a call are written by that call, not left over from the one in front"""
    for name in ("rows 2049 plain", "rows 257 rules", "list 2049", "rows 255 plain", "size 1 at one row", "rows 63 rules"):
        run(name)


@pytest.mark.gpu
@pytest.mark.parametrize("lib_name,guard", [("libwordpiece_amd_dbg.so", "0"), ("libwordpiece_amd.so", "1")])
def test_hardened_runs(tmp_path, lib_name, guard):
    """a fresh child on the bounds-checking build, and one under WP_ARENA_GUARD=1: no access outside an array or an arena"""
    lib = os.path.join(PKG, lib_name)
    assert os.path.exists(lib), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "scrub_edges_hard_run.py"
    script.write_text('''
import sys
import torch  # (before the library, as tests/conftest.py: the HIP runtime loaded first serves the process)
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_scrub_edges as T
v = T.handle()
v.encode("ab a")
assert v.stats()["reserved0"] == %d, "not the build this run is about"
for name in T.E.HARD:
    T.run(name)
print("SCRUB_EDGES_HARD_OK")
''' % (os.path.dirname(PKG), HERE, 1 if "dbg" in lib_name else 0))
    env = dict(os.environ, WP_LIB=lib, WP_ARENA_GUARD=guard)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "SCRUB_EDGES_HARD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
