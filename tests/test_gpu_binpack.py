"""wp_pack_best_fit / wp_pack_best_fit_device on the GPU against the literal procedure (tests/binpack_model.py): every
block and every statistic exactly.  The shapes sit at the kernels' edges (csrc/binpack.h): kBinTile = 1024 pieces per tile of
the hist pass and ranks per tile of the place pass (the radix sort's small tile too), tiles whose runs fit the LDS slice of
kBinRunSlice = 128 (5,000 mixed lengths at L = 128: 27 to 55 runs a tile) and tiles whose runs do not (1,023 to 1,025 of
them: 162 to 178 runs in the first tile), rows of 8192 units."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import binpack_model as M
import wordpiece_amd as W
from test_gpu_pack import CLS, KEYS, PAD, SEP, SPECIALS, VOCAB, ids_for, splits_of
from wordpiece_amd import binpack as B

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")


@pytest.fixture(scope="module")
def gv():
    return W.Vocab(VOCAB)


def check(gv, lens, L, long_docs="split", bos=-1, eos=-1, want=7):
    """the host and the device entry point on documents of the lengths `lens` against the model: blocks and statistics"""
    import torch
    splits = splits_of(lens)
    ids = ids_for(int(splits[-1]))
    exp = M.pack(ids, splits, L, bos, eos, PAD, M.PM.LONG_DOCS[long_docs], want)
    how = dict(max_len=L, bos_id=None if bos < 0 else bos, eos_id=None if eos < 0 else eos, pad_id=PAD, long_docs=long_docs, want=want)
    host = B.pack_best_fit(gv, ids, splits, **how)
    dev = B.pack_best_fit_tensor(gv, torch.as_tensor(ids, device="cuda"), torch.as_tensor(splits, device="cuda"), **how)
    assert B.binpack_stats(gv) == dict(exp["stats"], n_runs=len(B.plan_best_fit(exp["u"], L, lengths=True)["runs"]))
    for got in (host, {k: x.cpu().numpy() for k, x in dev.items()}):
        assert sorted(got) == sorted(k for k in KEYS if exp[k] is not None) and got["input_ids"].shape == (exp["n_out"], L)
        for k in got:
            if not np.array_equal(got[k], exp[k]):
                bad = np.argwhere(got[k] != exp[k])[0]
                raise AssertionError("%s differs at %s: %d != %d (%d cells differ; L %d, %s, bos %d, eos %d)" %
                                     (k, bad.tolist(), got[k][tuple(bad)], exp[k][tuple(bad)], int(np.sum(got[k] != exp[k])), L, long_docs, bos, eos))
    return exp


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2, 5, 128])
@pytest.mark.parametrize("n_p", [1, 2, 1023, 1024, 1025, 5000])
def test_piece_and_rank_tiles(gv, n_p, L):
    bos, eos = SPECIALS[(n_p + L) % 3] if L > 2 else (-1, -1)
    B_ = L - (bos >= 0) - (eos >= 0)
    exp = check(gv, np.random.default_rng(n_p * L).integers(1, B_ + 1, n_p), L, bos=bos, eos=eos)
    assert exp["stats"]["n_pieces"] == n_p


@pytest.mark.gpu
def test_rows_of_8192_units(gv):
    exp = check(gv, [1] * 20000, 8192)
    assert exp["n_out"] == 3 and exp["lengths"].tolist() == [8192, 8192, 20000 - 2 * 8192]


@pytest.mark.gpu
@pytest.mark.parametrize("bos,eos", SPECIALS)
@pytest.mark.parametrize("long_docs", ["truncate", "split"])
def test_long_and_empty_documents(gv, long_docs, bos, eos):
    B_ = 9 - (bos >= 0) - (eos >= 0)
    exp = check(gv, [0, 0, 2, 3 * B_ + 1, 0, 3, B_, 0, 5, 1, 0], 9, long_docs, bos, eos)
    assert exp["stats"]["n_empty"] == 5 and exp["stats"]["n_cut"] == (long_docs == "truncate")


@pytest.mark.gpu
@pytest.mark.parametrize("want", range(8))
def test_want(gv, want):
    check(gv, [3, 0, 6, 2, 9, 1], 8, "split", CLS, SEP, want)


@pytest.mark.gpu
def test_capacity_and_the_statistics_of_the_pack_call(gv):
    import torch
    lens = [5, 7, 3, 8, 8, 1, 2]
    splits = splits_of(lens)
    ids = ids_for(int(splits[-1]))
    gv.pack_sequences(ids, splits, max_len=8, eos_id=SEP)
    before = gv.pack_stats()
    exp = check(gv, lens, 8, eos=SEP)
    assert gv.pack_stats() == before and before["n_docs"] == len(lens)
    cap = exp["n_out"] - 1
    d_ids, d_splits = torch.as_tensor(ids, device="cuda"), torch.as_tensor(splits, device="cuda")
    bufs = {k: torch.full((cap,) if k == "lengths" else (cap, 8), -77, dtype=torch.int32, device="cuda") for k in KEYS}
    spec, n = B.BinpackSpec(8, -1, SEP, PAD, 1, 7, 0, 0), C.c_size_t()
    torch.cuda.synchronize()
    rc = B.lib().wp_pack_best_fit_device(gv._h, d_ids.data_ptr(), d_splits.data_ptr(), len(lens), C.byref(spec),
                                         C.byref(W.Packed(*[bufs[k].data_ptr() for k in KEYS])), cap, C.byref(n))
    assert rc == 6 and b"binpack: capacity_rows" in B.lib().wp_last_error() and n.value == exp["n_out"]
    assert all(bool((x == -77).all()) for x in bufs.values())
    out = B.pack_best_fit_tensor(gv, d_ids, d_splits, max_len=8, eos_id=SEP, pad_id=PAD, n_out=exp["n_out"])
    assert all(np.array_equal(out[k].cpu().numpy(), exp[k]) for k in KEYS)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"WP_LIB": os.path.join(PKG, "libwordpiece_amd_dbg.so")}, {"WP_ARENA_GUARD": "1"}], ids=["bounds", "guard"])
def test_checking_builds(tmp_path, env):
    script = tmp_path / "binpack_dbg_run.py"
    script.write_text('''
import os, sys
import torch  # (before the library, as tests/conftest.py: the HIP runtime loaded first serves the process)
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import wordpiece_amd as W
from test_gpu_binpack import VOCAB, check
gv = W.Vocab(VOCAB)
gv.encode("the cat")
assert gv.stats()["reserved0"] == int("WP_LIB" in os.environ), "not the build that was asked for"
check(gv, [0, 2, 25, 0, 3, 7, 1], 9, "split", 1, 2)
check(gv, np.random.default_rng(5).integers(1, 128, 1100), 128, eos=2)  # (more runs in the first tile than LDS holds)
print("BINPACK_DEBUG_OK")
''' % (os.path.dirname(PKG), HERE))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0 and "BINPACK_DEBUG_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
