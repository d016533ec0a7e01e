"""GPU checks of the seen-rows layer against tests/seen_model.py, exactly, in host and tensor form: the keys at the chunk
and tile edges of the key kernel, a sequence of calls on one handle, growth and reserve, crafted keys that wrap and
cluster, and one pass in the bounds-checking build and under WP_ARENA_GUARD=1."""
import os
import subprocess
import sys

import numpy as np
import pytest

import seen_model as M
import wordpiece_amd as W
from wordpiece_amd import seen as S

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")
VOCAB = ["[UNK]", "a", "b", "##b"]


def pattern(n, salt):
    return bytes((i * 7 + i // 251 + salt) & 0xff for i in range(n))


def call_rows(v, model, rows, tensor, ids=False, insert=True):
    """one batch through the library (keys and compact on) and through the model, every array compared with dtype and shape"""
    import torch
    data, eb = b"".join(rows), 4 if ids else 1
    off = (np.cumsum([0] + [len(r) for r in rows]) // eb).astype(np.int64)
    exp = model.add_rows(rows, insert)
    if tensor:
        t = torch.frombuffer(bytearray(data + b"\xff" * 8), dtype=torch.uint8).cuda()  # (dirty bytes behind the data)
        t = t.view(torch.int32)[:len(data) // 4] if ids else t[:len(data)]
        got = {k: x.cpu().numpy() for k, x in S.seen_rows_tensor(v, t, torch.from_numpy(off).cuda(), insert=insert, keys=True, compact=True).items()}
        assert got["keys"].dtype == np.int64
        got["keys"] = got["keys"].view(np.uint64)
    else:
        got = S.seen_rows(v, np.frombuffer(data, dtype=np.int32) if ids else data, off, insert=insert, keys=True, compact=True, raw=True)
    want = dict(state=np.array(exp["state"], np.int32), first=np.array(exp["first"], np.int32), keys=np.array(exp["keys"], np.uint64),
                kept=np.array(exp["kept"], np.int32), data=np.frombuffer(exp["data"], dtype=np.int32 if ids else np.uint8), row_off=np.array(exp["row_off"], np.int64) // eb)
    assert list(got) == list(want)
    for k, x in want.items():
        assert got[k].dtype == x.dtype and got[k].shape == x.shape and np.array_equal(got[k], x), (tensor, k, got[k][:8], x[:8])
    check_set(v, model, tensor)
    return exp


def call_keys(v, model, keys, tensor, insert=True):
    import torch
    exp = model.add_keys(keys, insert)
    keys = np.array(keys, dtype=np.uint64)
    if tensor:
        got = {k: x.cpu().numpy() for k, x in S.seen_add_keys_tensor(v, torch.from_numpy(keys.view(np.int64)).cuda(), insert=insert).items()}
    else:
        got = S.seen_add_keys(v, keys, insert=insert)
    assert list(got) == ["state", "first"] and all(got[k].dtype == np.int32 and got[k].tolist() == e for k, e in zip(got, exp)), (tensor, got, exp)
    check_set(v, model, tensor)
    return exp


def check_set(v, model, tensor):
    """the statistics of the last call and the export against the model"""
    st = S.seen_stats(v)
    assert {k: st[k] for k in model.stats} == model.stats and st["capacity"] >= 2 * st["n_keys"], st
    got = S.seen_keys_tensor(v).cpu().numpy().view(np.uint64) if tensor else S.seen_keys(v)
    assert got.dtype == np.uint64 and got.tolist() == model.export()


@pytest.mark.gpu
@pytest.mark.parametrize("tensor", [False, True], ids=["host", "tensor"])
@pytest.mark.parametrize("ids", [False, True], ids=["text", "ids"])
def test_keys_at_the_chunk_and_tile_edges(tensor, ids):
    """rows of every length around a word, a chunk and two chunks, and one a byte (an id) past the 256 x 256-byte tile of the key kernel"""
    lens = [0, 1, 3, 4, 5, 255, 256, 257, 512, 513, 65537]
    rows = [pattern(n * 4, n) for n in lens] if ids else [pattern(n, n) for n in lens]
    exp = call_rows(W.Vocab(VOCAB), M.Seen(), rows + rows[2:4], tensor, ids)
    assert exp["state"] == [0] * 11 + [1, 1] and exp["first"] == list(range(11)) + [2, 3]


def sequence(tensor):
    v, model = W.Vocab(VOCAB), M.Seen()
    a = [b"", b"one", b"two", b"", b"one", b"three" * 80, b"two", b"two"]  # runs whose smallest rows are 0, 1 and 2; empty rows
    b = [b"four", b"two", b"five", b"two", b"five", b"", b"six" * 200]    # "two" repeats inside b and is in a
    assert call_rows(v, model, a, tensor)["state"] == [0, 0, 0, 1, 1, 0, 1, 1]
    assert v.encode("ab a").tolist() == [1, 3, 1] and v.dedup_rows(b"x\ny\nx\n")["kept"].tolist() == [0, 1]  # other calls leave the set alone
    exp = call_rows(v, model, b, tensor)
    assert exp["state"] == [0, 2, 0, 2, 1, 2, 0] and exp["first"] == [0, 1, 2, 1, 2, 5, 6]
    W.lib().wp_trim(v._h)
    assert call_rows(v, model, a, tensor)["state"] == [2] * 8
    for _ in range(2):  # asking leaves the set as it is: the second answer is the first
        assert call_rows(v, model, [b"new", b"one", b"new", b"newer"], tensor, insert=False)["state"] == [0, 2, 1, 0]
    assert S.seen_stats(v)["n_keys"] == 7 and S.seen_docs(v, ["one", "seven", "seven"])[0] == [b"seven"]


def probing(tensor):
    v, model = W.Vocab(VOCAB), M.Seen()
    top = [(0xfffff << 44) | (i * 0x9e3779b1 & (1 << 44) - 1) for i in range(300)]  # home: the last slot of any table up to 2^20 slots
    mid = [(0x80001 << 44) | (i * 0x85ebca6b & (1 << 44) - 1) for i in range(300)]
    assert len(set(top + mid)) == 600
    assert call_keys(v, model, [0, 1], tensor) == ([0, 1], [0, 0])  # the key 0 is the key 1
    down = sorted(top + mid, reverse=True)
    assert call_keys(v, model, down, tensor)[0] == [0] * 600
    assert call_keys(v, model, top + mid + [1], tensor)[0] == [2] * 601
    S.seen_clear(v)
    model.keys.clear()
    assert S.seen_stats(v)["n_keys"] == 0 == S.seen_stats(v)["capacity"]
    assert call_keys(v, model, down, tensor)[0] == [0] * 600


@pytest.mark.gpu
@pytest.mark.parametrize("tensor", [False, True], ids=["host", "tensor"])
def test_a_sequence_of_calls_on_one_handle(tensor):
    sequence(tensor)


@pytest.mark.gpu
@pytest.mark.parametrize("tensor", [False, True], ids=["host", "tensor"])
def test_clusters_that_wrap_and_crowd(tensor):
    probing(tensor)


@pytest.mark.gpu
@pytest.mark.parametrize("tensor", [False, True], ids=["host", "tensor"])
def test_growth_and_reserve(tensor):
    batches = [[b"row %d of batch %d" % (i, k) for i in range(600)] for k in range(3)]
    for reserve in (False, True):
        v, model = W.Vocab(VOCAB), M.Seen()
        if reserve:
            S.seen_reserve(v, 10 ** 6)
        for k, rows in enumerate(batches):
            assert call_rows(v, model, rows, tensor)["state"] == [0] * 600
            # 1,024 slots at first; 2 x 600 keys ask for 2,048, 2 x 1,200 for 4,096, and 2 x 1,800 fit in those
            assert (S.seen_stats(v)["n_grown"], S.seen_stats(v)["capacity"]) == ((0, 1 << 21) if reserve else (min(k + 1, 2), (2048, 4096, 4096)[k]))
        assert call_rows(v, model, sum(batches, []), tensor, insert=False)["state"] == [2] * 1800


@pytest.mark.gpu
def test_more_runs_and_items_than_one_grid():
    """the lookup strides a grid of 2,048 workgroups of 32 probes, the states one of 2,048 x 256 items: a call past both"""
    rng = np.random.default_rng(5)
    base = rng.integers(1, 2 ** 63, 400000, dtype=np.uint64)
    keys = rng.permutation(np.concatenate((base, base[:130000]))).tolist()
    v, model = W.Vocab(VOCAB), M.Seen()
    exp = call_keys(v, model, keys, True)
    assert exp[0].count(0) == len(set(keys)) > 2048 * 32 and len(keys) > 2048 * 256
    assert call_keys(v, model, keys[::-1], True, insert=False)[0] == [2] * len(keys)


@pytest.mark.gpu
@pytest.mark.parametrize("lib_name,guard", [("libwordpiece_amd_dbg.so", "0"), ("libwordpiece_amd.so", "1")])
def test_hardened_runs(tmp_path, lib_name, guard):
    """a fresh child on the bounds-checking build, and one under WP_ARENA_GUARD=1: no access outside an array or an arena"""
    lib = os.path.join(PKG, lib_name)
    assert os.path.exists(lib), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "seen_hard_run.py"
    script.write_text('''
import sys
import torch  # (before the library, as tests/conftest.py: the HIP runtime loaded first serves the process)
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_seen as T
v = T.W.Vocab(T.VOCAB)
v.encode("ab a")
assert v.stats()["reserved0"] == %d, "not the build this run is about"
for tensor in (False, True):
    T.sequence(tensor)
    T.probing(tensor)
print("SEEN_HARD_OK")
''' % (os.path.dirname(PKG), HERE, 1 if "dbg" in lib_name else 0))
    env = dict(os.environ, WP_LIB=lib, WP_ARENA_GUARD=guard)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "SEEN_HARD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
