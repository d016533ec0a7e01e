"""GPU checks of the scrub against tests/scrub_model.py, exactly: every array of every want bit in both forms with its
dtype, and the statistics, over rows built around the kernel's edges: the tile, the runs of 64 / 255 / 16 bytes, the label
rules, the row ends, the private ranges, replacements that shrink and grow the text, a tile full of matches."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scrub_model as M
import wordpiece_amd as W
from wordpiece_amd import scrub as S

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")
T = 2048  # kQualTile (csrc/quality.h): the bytes of a tile of both kernels
ARRAYS = (("signals", np.int64), ("reasons", np.uint32), ("match_row", np.int32), ("match_start", np.int64), ("match_len", np.int32), ("match_kind", np.int32),
          ("match_repl", np.int32), ("out_data", np.uint8), ("out_off", np.int64), ("kept", np.int32), ("data", np.uint8), ("row_off", np.int64))
E16 = [b"<mail %d>" % k + b"." * k for k in range(16)]
DOMAIN = b"a" * 63 + b"." + b"b" * 63 + b"." + b"c" * 63 + b"."  # 192 bytes; the last label brings it to 255 or 256
RANGES = b" ".join(b"%d.%d.%d.%d" % a for a in ((0, 0, 0, 0), (0, 255, 255, 255), (1, 0, 0, 0), (10, 0, 0, 0), (10, 255, 255, 255), (11, 0, 0, 0), (127, 0, 0, 0),
                                                (127, 255, 255, 255), (128, 0, 0, 0), (169, 254, 0, 0), (169, 254, 255, 255), (169, 255, 0, 0), (172, 16, 0, 0),
                                                (172, 31, 255, 255), (172, 32, 0, 0), (192, 168, 0, 0), (192, 168, 255, 255), (192, 169, 0, 0), (223, 255, 255, 255),
                                                (224, 0, 0, 0), (255, 255, 255, 255)))
sp = lambda n: b" " * n  # noqa: E731
CASES = {
    # one row, so that positions in it are positions in the batch: the '@' at 1, T - 1, 2 T (position 0, or T of the tile in front) and 3 T + 1
    "@ at tile positions 0, 1, T-1, T": ([b"a@cd.ee" + sp(T - 10) + b"ab@cd.ee" + sp(T - 7) + b"ab@cd.ee" + sp(T - 7) + b"ab@cd.ee"], {}),
    # the '@' lie at T + 24, 2 T + 16 and 3 T + 34: each run in front of them began in the tile in front
    "local runs of 64 and 65 over a tile start": ([sp(T - 40) + b"x" * 64 + b"@cd.ee " + sp(T - 80) + b"y" * 65 + b"@cd.ee", sp(T - 52) + b"%" + b"z" * 63 + b"@cd.ee"], {}),
    "domain runs of 255 and 256 over a tile end": ([sp(T - 100) + b"u@" + DOMAIN + b"d" * 60 + b".ee " + sp(T - 300) + b"u@" + DOMAIN + b"d" * 61 + b".ee"], {}),
    "labels": ([b"x@" + b"a" * 63 + b".com x@" + b"a" * 64 + b".com x@-a.com x@a-.com x@a.b-.com x@a..com x@a.com.-b x@a.c x@a.B1.Cd.e2"], dict(email=E16)),
    "an address over a tile edge": ([sp(T - 1) + b"8.8.8.8 " + sp(T - 12) + b"9.9.9.9"], dict(ip=[b"i"])),
    "NUM runs and octets": ([b"100.100.100.100. 100.100.100.100.. 1.2.3.255 1.2.3.256 01.2.3.4 0.0.0.0 1.2.3.4.5 1..2.3 .1.2.3.4 1.2.3.4x \xc3\xa91.2.3.4 _1.2.3.4"], {}),
    "row ends": ([b"abc", b"@de.ff", b"abc@", b"de.ff", b"1.2.", b"3.4", b"x@y.zz", b"1.2.3.4", b"a@b.c", b"c a@b.cc", b"", b"1.2.3.4"], {}),
    "private ranges replaced": ([RANGES], {}),
    "private ranges left": ([RANGES, b"1.2.3.4@x.org 10.1.1.1-x@y.org"], dict(keep_private=True)),
    "replacements of 0, 1 and 64 bytes": ([b"to a@b.cc and 8.8.8.8, " * 150], dict(email=[b""], ip=[b"E" * 64, b"i"])),
    "hash fold and a list of 16": ([b"Bob@Example.COM bob@example.com " + b" ".join(b"u%d@h%d.org" % (k, k) for k in range(60))], dict(email=E16, ip=[b"i"])),
    "a tile of minimal matches": ([b"a@b.cc " * 700], dict(email=[b"<e>", b""])),
    "no match, empty rows": ([b"", b"plain text @ 1.2.3 here " * 120, b"", b""], {}),
    "e-mails only": ([b"a@b.cc 8.8.8.8"], dict(kinds=["email"])),
    "addresses only": ([b"a@b.cc 8.8.8.8 1.2.3.4@b.cc"], dict(kinds=["ipv4"])),
}
for a in range(4):  # the shift between input and output takes every phase of a word (+1, +4 a line), from every phase of the tile
    CASES["alignment %d" % a] = ([sp(a) + b"mail a@b.cc or 10.0.0.1 now. " * 160], dict(email=[b"e-mail."], ip=[b"<an address>"]))
HARD = ("a tile of minimal matches", "domain runs of 255 and 256 over a tile end", "replacements of 0, 1 and 64 bytes", "row ends")
_handle = []


def handle():
    if not _handle:
        _handle.append(W.Vocab(["[UNK]", "a", "b"]))
    return _handle[0]


def check(rows, how, where):
    """the rows through both forms against the model -> the model's answer"""
    import torch
    v = handle()
    data, off = b"".join(rows), np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    default = S.scrub_replacements("default")
    kinds = sum(1 << S.SCRUB_KINDS.index(k) for k in how.get("kinds", ("email", "ipv4"))) | (M.KEEP_PRIVATE if how.get("keep_private") else 0)
    exp = M.scrub_rows(data, off.tolist(), kinds, [W._bytes(x) for x in how.get("email", default["email"])], [W._bytes(x) for x in how.get("ip", default["ip"])],
                       how.get("rules"))
    for tensor in (False, True):
        if tensor:
            t = torch.frombuffer(bytearray(data + b"@\xff\xff\xff"), dtype=torch.uint8).cuda()[:len(data)]  # (dirty bytes behind the data)
            got = S.scrub_rows_tensor(v, t, torch.from_numpy(off).cuda(), matches=True, text=True, compact=True, **how)
            got = {k: x.cpu().numpy() for k, x in got.items()}
            assert got["reasons"].dtype == np.int32
            got["reasons"] = got["reasons"].view(np.uint32)
        else:
            got = S.scrub_rows(v, data, off, matches=True, text=True, compact=True, raw=True, **how)
        for key, dtype in ARRAYS:
            want = np.frombuffer(exp[key], dtype=np.uint8) if dtype == np.uint8 else np.asarray(exp[key], dtype=dtype).reshape((8, len(rows)) if key == "signals" else -1)
            assert got[key].dtype == dtype and got[key].shape == want.shape, (where, tensor, key, got[key].dtype, got[key].shape, want.shape)
            bad = np.argwhere(got[key] != want)[:6]
            assert not len(bad), (where, tensor, key, [(tuple(map(int, i)), int(got[key][tuple(i)]), int(want[tuple(i)])) for i in bad])
        assert S.scrub_stats(v) == exp["stats"] and len(got) == len(ARRAYS), (where, tensor, S.scrub_stats(v), exp["stats"])
    return exp


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_array_against_the_model(name):
    rows, how = CASES[name]
    exp = check(rows, how, name)
    ats = [b"".join(rows).find(b"@", s) for s in exp["match_start"]]  # where the '@' of the e-mail matches lie in the batch
    if name.startswith("@ at"):
        assert ats == [1, T - 1, 2 * T, 3 * T + 1]
    if name.startswith("local runs"):  # the run of 65 is no match; the others begin 40 and 29 bytes in front of a tile start
        assert ats == [T + 24, 3 * T + 34] and exp["match_start"] == [T - 40, 3 * T - 29]
    n = {"@ at tile positions 0, 1, T-1, T": [4, 0, 0], "local runs of 64 and 65 over a tile start": [2, 0, 0], "domain runs of 255 and 256 over a tile end": [1, 0, 0],
         "labels": [3, 0, 0], "an address over a tile edge": [0, 2, 0], "NUM runs and octets": [0, 3, 0], "row ends": [2, 2, 0], "private ranges replaced": [0, 21, 0],
         "private ranges left": [2, 7, 14], "a tile of minimal matches": [700, 0, 0], "no match, empty rows": [0, 0, 0]}.get(name)
    assert n is None or exp["stats"]["n_matches"] == n
    if name == "hash fold and a list of 16":  # one placeholder for both spellings; the list is used widely
        assert exp["match_repl"][0] == exp["match_repl"][1] and len(set(exp["match_repl"])) > 4
    if name.startswith("alignment"):
        assert exp["stats"]["n_out_bytes"] == exp["stats"]["n_bytes"] + 160 * 5 and exp["stats"]["n_bytes"] > 2 * T


@pytest.mark.gpu
def test_both_rules_at_equality_and_one_past():
    rows = [b"a@b.cc c@d.ee", b"8.8.8.8 10.0.0.1", b"none"]
    exp = check(rows, dict(rules={"max_emails": 2, "max_ips": 2}, keep_private=True), "at equality")
    assert exp["reasons"] == [0, 0, 0] and exp["signals"][M.S["ips_left"]] == [0, 1, 0]
    exp = check(rows, dict(rules={"max_emails": 1, "max_ips": 1}, keep_private=True), "one past")
    assert exp["reasons"] == [1, 2, 0] and exp["kept"] == [2]
    for want in ({}, {"matches": True}, {"text": True}, {"compact": True}):  # every form alone hands out its own arrays and no other
        got = S.scrub_rows(handle(), b"".join(rows), [0, 13, 29, 33], **want)
        assert len(got) == 2 + {"": 0, "matches": 5, "text": 2, "compact": 3}["".join(want)] and got["reasons"].tolist() == [0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("lib_name,guard", [("libwordpiece_amd_dbg.so", "0"), ("libwordpiece_amd.so", "1")])
def test_hardened_runs(tmp_path, lib_name, guard):
    """a fresh child on the bounds-checking build, and one under WP_ARENA_GUARD=1: no access outside an array or an arena"""
    lib = os.path.join(PKG, lib_name)
    assert os.path.exists(lib), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "scrub_hard_run.py"
    script.write_text('''
import sys
import torch  # (before the library, as tests/conftest.py: the HIP runtime loaded first serves the process)
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_scrub as T
v = T.handle()
v.encode("ab a")
assert v.stats()["reserved0"] == %d, "not the build this run is about"
for name in T.HARD:
    T.test_every_array_against_the_model(name)
print("SCRUB_HARD_OK")
''' % (os.path.dirname(PKG), HERE, 1 if "dbg" in lib_name else 0))
    env = dict(os.environ, WP_LIB=lib, WP_ARENA_GUARD=guard)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "SCRUB_HARD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
