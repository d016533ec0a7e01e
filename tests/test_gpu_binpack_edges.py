"""Best-fit packing past its first grid (csrc/binpack.h, binpack_path.h), exactly against tests/binpack_model.py through
test_gpu_binpack.check: every block of both entry points and every statistic.

  1  binpack_hist_kernel's grid-stride loop takes a second and a third step: kBinHistGrid * kBinTile + 1 pieces, and a size at
     which some workgroups take three tiles and others two.  L = 4 and 5 with random lengths 1 .. L: equal lengths among a
     lane's four items are common (the run folding), and the full unit stands in every wave (the ballot).
  2  the ballot over the full units (u == L): at one lane of a wave only (lane 0, 63, 29), at every lane of a wave, in the last,
     partial wave of the last tile only, at every subset of a lane's four items; long_docs "split", where the full units are the
     chunks of long documents, and "truncate" over the same documents; L = 3 and 8, with and without bos / eos.
  3  the LDS histogram at its full size: L = 8192 with lengths in [1, kBlock], (kBlock, 2 kBlock], around 4096, L - 1 and L;
     L = kBlock - 1, kBlock, kBlock + 1 with every length present (the clear and the flush loops end in a partial step).
  4  binpack_place_kernel's run slice: kBinRunSlice - 1, kBinRunSlice and kBinRunSlice + 1 runs in the first rank tile (the
     last that LDS holds, the first that is searched in global memory), and a batch whose last, partial tile alone exceeds it.

The model on the CPU (tests/binpack_model.py, one core): pack() takes 0.9 s for the 524,289 pieces of group 1 and 2.4 s for
the 1,049,603 (place() 0.65 s and 1.5 s of it), so both sizes stay in the -m gpu run, as the sizes of test_gpu_fullsize.py do;
every other case of this file together 0.25 s.  Wall time on an MI355X: 4.2 s for the 39 tests of this file.  Found by this file:
nothing.  With the `tile += gridDim.x` loop of binpack_hist_kernel stopped after its first tile, test_gpu_binpack.py passes and
test_hist_grid_takes_further_steps fails at both sizes (the host's sum check over the histogram throws)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_binpack import HERE, PKG, check, gv  # noqa: F401  (gv: the fixture)
from test_gpu_pack import CLS, SEP
from wordpiece_amd import binpack as B

BLOCK, WAVE, ITEMS, GRID, SLICE, MAX_LEN = 256, 64, 4, 512, 128, 8192
TILE = BLOCK * ITEMS  # kBinTile: the pieces of a tile of the hist pass, the ranks of a tile of the place pass
SPECIALS = ((-1, -1), (CLS, SEP))


def test_geometry_the_cases_are_built_from():
    src = open(os.path.join(PKG, "csrc", "binpack.h")).read()
    common = open(os.path.join(PKG, "csrc", "common.h")).read()
    hdr = open(os.path.join(os.path.dirname(PKG), "include", "wordpiece_amd_binpack.h")).read()
    value = lambda text, name: re.search(r"^constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, text, re.M).group(1).strip()  # noqa: E731
    assert (int(value(common, "kBlock")), int(value(common, "kWave"))) == (BLOCK, WAVE)
    assert int(value(src, "kBinItems")) == ITEMS and value(src, "kBinTile") == "kBlock * kBinItems" and TILE == 1024
    assert int(value(src, "kBinHistGrid")) == GRID and int(value(src, "kBinRunSlice")) == SLICE and value(src, "kBinMaxLen") == "WP_BINPACK_MAX_LEN"
    assert int(re.search(r"#define WP_BINPACK_MAX_LEN\s+(\d+)", hdr).group(1)) == MAX_LEN == B.WP_BINPACK_MAX_LEN


# ---- 1. the strided histogram ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_p,L,eos", [(GRID * TILE + 1, 4, -1), (2 * GRID * TILE + TILE + 3, 5, SEP)], ids=["second step", "two and three steps"])
def test_hist_grid_takes_further_steps(gv, n_p, L, eos):
    """workgroup 0 takes a second tile of one piece; workgroups 0 and 1 take a third tile, the others two"""
    exp = check(gv, np.random.default_rng(n_p).integers(1, L + (eos < 0), n_p), L, eos=eos)
    hist = np.bincount(exp["u"], minlength=L + 1)
    assert exp["stats"]["n_pieces"] == n_p > GRID * TILE and hist[1 + (eos >= 0):].min() > n_p // 8, hist  # the full unit is as common as the others


# ---- 2. the full units in every wave shape --------------------------------------------------------------------------------------
def piece(tile, wave, lane, item):
    return tile * TILE + (wave * WAVE + lane) * ITEMS + item


ARRANGEMENTS = {
    "lane 0": (TILE + 77, [piece(0, w, 0, w) for w in range(4)]),        # one full unit a wave, in the ballot of another item each
    "lane 63": (TILE + 77, [piece(0, w, 63, w) for w in range(4)]),
    "lane 29": (TILE + 77, [piece(0, w, 29, 3 - w) for w in range(4)]),
    "every lane of a wave": (TILE, list(range(piece(0, 2, 0, 0), piece(0, 3, 0, 0)))),
    "last partial wave": (TILE + BLOCK + 42, [TILE + BLOCK + k for k in (1, 5, 41)]),  # tile 1: wave 0 whole, wave 1 of ten lanes and two items
    "items of a lane": (TILE, [piece(0, 0, t, j) for t in range(BLOCK) for j in range(ITEMS) if t % 16 >> j & 1]),
}


def documents(n_p, full, L, s):
    """-> (the document lengths, the units of the pieces under long_docs "split"): piece k has L units where k is in `full`
    and fewer elsewhere; every run of full pieces and the piece behind it are the chunks of one long document"""
    B_ = L - s
    if B_ < 2:  # (a budget of one id: every piece is full)
        return [n_p * B_], np.full(n_p, L)
    u = np.random.default_rng(n_p + L).integers(s + 1, L, n_p)
    u[full] = L
    lens, run = [], 0
    for x in u.tolist():
        if x == L:
            run += 1
        else:
            lens.append(run * B_ + x - s)
            run = 0
    return lens + [run * B_] * (run > 0), u


@pytest.mark.gpu
@pytest.mark.parametrize("bos,eos", SPECIALS, ids=["plain", "bos eos"])
@pytest.mark.parametrize("L", [3, 8])
@pytest.mark.parametrize("name", sorted(ARRANGEMENTS))
def test_full_units_in_every_wave_shape(gv, name, L, bos, eos):
    n_p, full = ARRANGEMENTS[name]
    s = (bos >= 0) + (eos >= 0)
    lens, u = documents(n_p, full, L, s)
    exp = check(gv, lens, L, "split", bos, eos)
    assert np.array_equal(exp["u"], u) and (L - s < 2 or np.flatnonzero(exp["u"] == L).tolist() == sorted(full))
    exp = check(gv, lens, L, "truncate", bos, eos)  # every long document gives one full piece
    long_ = [x > L - s for x in lens]
    assert exp["stats"]["n_cut"] == sum(long_) and np.array_equal(exp["u"] == L, np.asarray(lens) >= L - s)


# ---- 3. the LDS histogram at its full size --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("eos", [-1, SEP])
def test_every_range_of_the_largest_histogram(gv, eos):
    L = MAX_LEN
    around = list(range(L // 2 - 6, L // 2 + 7))
    lens = list(range(1, BLOCK + 1, 3)) + list(range(BLOCK + 1, 2 * BLOCK + 1, 3)) + [BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1] + \
        around * 2 + [L - 2] * 3 + [L - 1] * 5 + [L] * 5 + [2 * L + 5]
    lens = np.random.default_rng(L).permutation(lens)
    exp = check(gv, lens, L, eos=eos)
    bins = np.flatnonzero(np.bincount(exp["u"], minlength=L + 1))
    assert len(lens) > 200 and {1 + (eos >= 0), BLOCK, BLOCK + 1, 2 * BLOCK, L // 2, L - 1, L} <= set(bins.tolist()) and len(bins) > 180


@pytest.mark.gpu
@pytest.mark.parametrize("L", [BLOCK - 1, BLOCK, BLOCK + 1])
def test_every_length_at_the_workgroup_edge(gv, L):
    rng = np.random.default_rng(L)
    exp = check(gv, rng.permutation(np.concatenate([np.arange(1, L + 1), rng.integers(1, L + 1, 2 * L)])), L)
    assert np.bincount(exp["u"], minlength=L + 1)[1:].min() >= 1


# ---- 4. the run slice -----------------------------------------------------------------------------------------------------------
def runs_of_tiles(u, L):
    """the plan of the units -> the runs every rank tile's slice holds"""
    first = B.plan_best_fit(u, L, lengths=True)["runs"]["first_rank"]
    return [int(np.searchsorted(first, min(i0 + TILE, len(u)) - 1, "right") - np.searchsorted(first, i0, "right")) + 1 for i0 in range(0, len(u), TILE)]


SLICES = {SLICE - 1: 6, SLICE: 2, SLICE + 1: 13}  # the seed whose 1,300 lengths of 1 .. 128 give the first tile that many runs


def last_tile_units():
    return np.concatenate([[100] * TILE, [90] * TILE, [80] * TILE, np.random.default_rng(5).integers(1, 127, 1020)])  # 27, 11, 11 and 137 runs


def test_run_slice_batches_are_what_they_claim():
    """(the planner alone, no GPU) the counts the place pass will see"""
    for n_runs, seed in SLICES.items():
        assert runs_of_tiles(np.random.default_rng(seed).integers(1, 129, 1300), 128)[0] == n_runs
    per_tile = runs_of_tiles(last_tile_units(), 128)
    assert len(per_tile) == 4 and max(per_tile[:3]) < SLICE < per_tile[3], per_tile


@pytest.mark.gpu
@pytest.mark.parametrize("n_runs", sorted(SLICES))
def test_run_slice_at_its_size(gv, n_runs):
    u = np.random.default_rng(SLICES[n_runs]).integers(1, 129, 1300)
    assert runs_of_tiles(u, 128)[0] == n_runs
    exp = check(gv, u, 128)
    assert np.array_equal(exp["u"], u)


@pytest.mark.gpu
def test_only_the_last_partial_tile_exceeds_the_slice(gv):
    u = last_tile_units()
    per_tile = runs_of_tiles(u, 128)
    assert max(per_tile[:3]) < SLICE < per_tile[3] and len(u) % TILE
    check(gv, np.random.default_rng(1).permutation(u), 128)


# ---- the checking builds --------------------------------------------------------------------------------------------------------
def cheapest_of_every_group(gv):
    """(the child of test_checking_builds) one case of each group, none of the 524,289-piece ones"""
    for name in ("lane 63", "last partial wave", "items of a lane"):
        lens, _ = documents(*ARRANGEMENTS[name], 8, 2)
        check(gv, lens, 8, "split", CLS, SEP)
        check(gv, lens, 8, "truncate", CLS, SEP)
    test_every_range_of_the_largest_histogram(gv, SEP)
    test_every_length_at_the_workgroup_edge(gv, BLOCK + 1)
    for n_runs in SLICES:
        test_run_slice_at_its_size(gv, n_runs)
    test_only_the_last_partial_tile_exceeds_the_slice(gv)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"WP_LIB": os.path.join(PKG, "libwordpiece_amd_dbg.so")}, {"WP_ARENA_GUARD": "1"}], ids=["bounds", "guard"])
def test_checking_builds(tmp_path, env):
    script = tmp_path / "binpack_edges_dbg_run.py"
    script.write_text('''
import os, sys
import torch  # (before the library, as tests/conftest.py: the HIP runtime loaded first serves the process)
sys.path.insert(0, %r); sys.path.insert(0, %r)
import wordpiece_amd as W
import test_gpu_binpack_edges as T
from test_gpu_binpack import VOCAB
gv = W.Vocab(VOCAB)
gv.encode("the cat")
assert gv.stats()["reserved0"] == int("WP_LIB" in os.environ), "not the build that was asked for"
T.cheapest_of_every_group(gv)
print("BINPACK_EDGES_DEBUG_OK")
''' % (os.path.dirname(PKG), HERE))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0 and "BINPACK_EDGES_DEBUG_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
