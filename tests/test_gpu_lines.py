"""GPU checks of the line filter against tests/lines_model.py, exactly: every array of both forms with its dtype, the cut,
the compact form and the statistics, over tests/lines_cases.py; every rule at equality and one past it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lines_cases as K
import lines_model as M
import wordpiece_amd as W
from wordpiece_amd import lines as L

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")
ARRAYS = (("signals", np.int64), ("reasons", np.uint32), ("line_row", np.int32), ("line_start", np.int64), ("line_len", np.int32), ("line_reasons", np.uint32),
          ("cut_data", np.uint8), ("cut_off", np.int64), ("kept", np.int32), ("data", np.uint8), ("row_off", np.int64))
_handle = []


def handle():
    if not _handle:
        _handle.append(W.Vocab(["[UNK]", "a", "b"]))
    return _handle[0]


def check(rows, how, where):
    """the rows through both forms against the model -> the model's answer"""
    import torch
    v = handle()
    data, off = K.join(rows)
    exp = M.filter_lines(data, off.tolist(), **how)
    for tensor in (False, True):
        if tensor:
            t = torch.frombuffer(bytearray(data + b"\xff" * 4), dtype=torch.uint8).cuda()[:len(data)]  # (a dirty byte behind the data)
            got = L.filter_lines_tensor(v, t, torch.from_numpy(off).cuda(), lines=True, cut=True, compact=True, **how)
            got = {k: x.cpu().numpy() for k, x in got.items()}
            for key in ("reasons", "line_reasons"):
                assert got[key].dtype == np.int32
                got[key] = got[key].view(np.uint32)
        else:
            got = L.filter_lines(v, data, off, lines=True, cut=True, compact=True, raw=True, **how)
        for key, dtype in ARRAYS:
            want = np.frombuffer(exp[key], dtype=np.uint8) if dtype == np.uint8 else np.asarray(exp[key], dtype=dtype).reshape((15, len(rows)) if key == "signals" else -1)
            assert got[key].dtype == dtype and got[key].shape == want.shape, (where, tensor, key, got[key].dtype, got[key].shape, want.shape)
            bad = np.argwhere(got[key] != want)[:6]
            assert not len(bad), (where, tensor, key, [(tuple(map(int, i)), int(got[key][tuple(i)]), int(want[tuple(i)])) for i in bad])
        assert L.lines_stats(v) == exp["stats"] and len(got) == len(ARRAYS), (where, tensor, L.lines_stats(v), exp["stats"])
    return exp


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_every_array_against_the_model(name):
    rows, how = K.CASES[name]()
    exp = check(rows, how, name)
    if name.startswith("match ") or name == "upper case":  # both occurrences are found, whichever tile they end in
        assert exp["stats"]["n_phrase_matches"] == 2
    if name == "cut by a row end":
        assert exp["stats"]["n_phrase_matches"] == 2 and exp["signals"][M.S["doc_phrase_hits"]] == [0, 1, 0]
    if name == "a wave of matches":
        assert exp["signals"][M.S["doc_phrase_hits"]] == [65, 600, 0]
    if name.startswith("cut phase"):  # the second tile's first kept byte lands on every phase of a word
        assert exp["stats"]["n_bytes"] - exp["stats"]["n_kept_bytes"] == int(name[-1]) + 11 and exp["cut_off"][1] > K.T
    if name == "dups in the batch":
        assert exp["stats"]["line_failed"][5] == 7


@pytest.mark.gpu
def test_every_rule_at_equality_and_one_past():
    rows = [b"a b c.\nd e\nfour long words here...\n", b"spam {\nok.\n"]
    at = dict(rules={"min_words": 2, "min_chars": 3, "min_kept_lines": 2, "min_kept_words": 9, "max_dropped_x1000": 0, "max_doc_phrase_hits": 1}, doc_phrases=[b"{"])
    exp = check(rows, at, "at equality")
    assert exp["line_reasons"] == [0] * 5 and exp["reasons"] == [0, 1 << 1]
    past = dict(at, rules={"min_words": 3, "min_chars": 4, "min_kept_lines": 2, "min_kept_words": 5, "max_dropped_x1000": 93, "max_doc_phrase_hits": 0})
    exp = check(rows, past, "one past")
    assert exp["line_reasons"] == [0, 3, 0, 1, 3] and exp["reasons"] == [4, 1 | 2 | 4 | 8]
    exp = check(rows, dict(rules={"not_terminal": 0, "ellipsis_end": 0, "max_dropped_x1000": 100}), "the flag rules")
    assert exp["line_reasons"] == [0, 4, 8, 4, 0] and exp["reasons"] == [4, 4]
    for want in ({}, {"lines": True}, {"cut": True}, {"compact": True}):  # every form alone hands out its own arrays and no other
        got = L.filter_lines(handle(), *K.join(rows), rules={"not_terminal": 0}, **want)
        assert len(got) == 2 + {"": 0, "lines": 4, "cut": 2, "compact": 3}["".join(want)] and got["reasons"].tolist() == [0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("lib_name,guard", [("libwordpiece_amd_dbg.so", "0"), ("libwordpiece_amd.so", "1")])
def test_hardened_runs(tmp_path, lib_name, guard):
    """a fresh child on the bounds-checking build, and one under WP_ARENA_GUARD=1: no access outside an array or an arena"""
    lib = os.path.join(PKG, lib_name)
    assert os.path.exists(lib), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "lines_hard_run.py"
    script.write_text('''
import sys
import torch  # (before the library, as tests/conftest.py: the HIP runtime loaded first serves the process)
sys.path.insert(0, %r); sys.path.insert(0, %r)
import lines_cases as K
import test_gpu_lines as T
v = T.handle()
v.encode("ab a")
assert v.stats()["reserved0"] == %d, "not the build this run is about"
for name in K.HARD:
    T.test_every_array_against_the_model(name)
print("LINES_HARD_OK")
''' % (os.path.dirname(PKG), HERE, 1 if "dbg" in lib_name else 0))
    env = dict(os.environ, WP_LIB=lib, WP_ARENA_GUARD=guard)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "LINES_HARD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
