"""GPU checks of the repetition signals against tests/repetition_model.py, exactly: every array of both forms with its
dtype, the compact form and the statistics, over tests/repetition_cases.py; every rule at equality and one past it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import repetition_cases as K
import repetition_model as M
import wordpiece_amd as W
from wordpiece_amd import repetition as R

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")
_handle = []


def handle():
    if not _handle:
        _handle.append(W.Vocab(["[UNK]", "a", "b"]))
    return _handle[0]


def check(rows, rules, where, compact=True):
    """the rows through both forms against the model -> the model's answer"""
    import torch
    v = handle()
    data, off = K.join(rows)
    exp = M.repetition(data, off.tolist(), limit=M.limits(**rules))
    for tensor in (False, True):
        if tensor:
            t = torch.frombuffer(bytearray(data + b"\xff" * 4), dtype=torch.uint8).cuda()[:len(data)]  # (a dirty byte behind the data)
            got = R.repetition_rows_tensor(v, t, torch.from_numpy(off).cuda(), rules=rules, compact=compact)
            got = {k: x.cpu().numpy() for k, x in got.items()}
            assert got["reasons"].dtype == np.int32
            got["reasons"] = got["reasons"].view(np.uint32)
        else:
            got = R.repetition_rows(v, data, off, rules=rules, compact=compact, raw=True)
        for key, dtype, want in (("signals", np.int64, np.asarray(exp["signals"], dtype=np.int64).reshape(14, len(rows))), ("reasons", np.uint32, exp["reasons"]),
                                 ("kept", np.int32, exp["kept"]), ("row_off", np.int64, exp["row_off"]),
                                 ("data", np.uint8, np.frombuffer(exp["data"], dtype=np.uint8)))[:5 if compact else 2]:
            want = np.asarray(want, dtype=dtype)
            assert got[key].dtype == dtype and got[key].shape == want.shape, (where, tensor, key, got[key].dtype, got[key].shape, want.shape)
            bad = np.argwhere(got[key] != want)[:6]
            assert not len(bad), (where, tensor, key, [(tuple(map(int, i)), int(got[key][tuple(i)]), int(want[tuple(i)])) for i in bad])
        assert R.repetition_stats(v) == exp["stats"] and len(got) == (5 if compact else 2), (where, tensor, sorted(got))
    return exp


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_every_array_against_the_model(name):
    exp = check(K.CASES[name](), M.GOPHER, name)
    if name == "seam":  # equal neighbours share nothing; the row that joins them repeats itself
        assert exp["signals"][M.S["dup_5_chars"]] == [0, 0, 6, 0, 0]
    if name == "agree":  # m = 9: a duplicate at n = 9, none at n = 10; m = 10, 11: one at n = 10
        assert [s > 0 for s in exp["signals"][M.S["dup_10_chars"]]] == [False] * 9 + [True] * 2 and exp["signals"][M.S["dup_9_chars"]][8] > 0
    if name == "ties":
        assert [exp["signals"][M.S["top_2_chars"]][i] for i in (0, 1)] == [8, 8]


@pytest.mark.gpu
def test_every_rule_at_equality_and_one_past():
    rows = K.CASES["rules"]()
    at = check(rows, K.RULES_AT, "at equality")
    past = check(rows, {k: x - 1 for k, x in K.RULES_AT.items()}, "one past")
    assert at["reasons"] == [0] * 9 and all(past["reasons"][k] >> k & 1 for k in range(9)) and past["stats"]["n_kept"] == 0
    one = check(rows, {"max_dup_7_chars": 249}, "one rule alone")
    assert all(r in (0, 1 << 5) for r in one["reasons"]) and one["stats"]["rule_failed"][5] == sum(1 for r in one["reasons"] if r)
    check(rows, {"max_dup_7_chars": 249}, "without the compact form", compact=False)  # (the two arrays alone, the same kept count)


@pytest.mark.gpu
@pytest.mark.parametrize("lib_name,guard", [("libwordpiece_amd_dbg.so", "0"), ("libwordpiece_amd.so", "1")])
def test_hardened_runs(tmp_path, lib_name, guard):
    """a fresh child on the bounds-checking build, and one under WP_ARENA_GUARD=1: no access outside an array or an arena"""
    lib = os.path.join(PKG, lib_name)
    assert os.path.exists(lib), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "repetition_hard_run.py"
    script.write_text('''
import sys
import torch  # (before the library, as tests/conftest.py: the HIP runtime loaded first serves the process)
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_repetition as T
v = T.handle()
v.encode("ab a")
assert v.stats()["reserved0"] == %d, "not the build this run is about"
for name in ("row sizes", "word tile edges", "byte tile edges", "three tiles", "random 0", "multibyte"):
    T.test_every_array_against_the_model(name)
print("REPETITION_HARD_OK")
''' % (os.path.dirname(PKG), HERE, 1 if "dbg" in lib_name else 0))
    env = dict(os.environ, WP_LIB=lib, WP_ARENA_GUARD=guard)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "REPETITION_HARD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
