"""GPU checks of the byte-level BPE encoder against tests/bpe_model.py: every array of both forms, exactly, over one batch
built around the kernels' sizes (csrc/bpe.h): the byte tile T of the class and start pass, the bounds SHORT and MEDIUM of the
three merge paths, the 64-lane and 256-lane chunks of the cooperative loop, and the 256 rows of a block of the row kernels."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bpe_model as M
import wordpiece_amd as W
from wordpiece_amd import bpe as B

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")
T, SHORT, MEDIUM = B.TILE_BYTES, B.SHORT_BYTES, B.MEDIUM_BYTES
fill = lambda n: (b"ab cd, " * (n // 7 + 1))[:n]  # noqa: E731
EDGE = " we'll's \U0001f600 x'd　é'".encode()  # a start, a U+0020 prefix, contractions, a 4-byte character: each byte on either side of a tile edge
BOUNDS = [b - 1 + k for b in (SHORT, MEDIUM) for k in range(3)]
CHAIN = b"bcdefghijklmnopqrstuvwxyz"  # model "hand": a merge per byte, each on the result of the one before
DOCS = ([b"", b""] + [fill(T - s) + EDGE + fill(T + s - len(EDGE)) for s in range(1, len(EDGE) + 1)]  # (every document here is 2 T bytes: the edges stay where they are)
        + [b"x" * n for n in BOUNDS] + [b"a" * n for n in BOUNDS + [3 * 256 + 5]] + [b"q" + b" " * n for n in BOUNDS] + [b"x" + b"a" * 131 + b" " + b"a" * 64 + b"ba" * 9]
        + [b"z", b"", b"", b"\xff\xc3\xe4\xb8\x80\xf0\x9f\x98", b"\xe4\xb8", b"\xad caf\xc3", b"\xa9", CHAIN, CHAIN[:SHORT], b" " + CHAIN * 11, b"  \t\n", b"it's 12th\xc2\xa0  \n\n x"]
        + [b"h"] * 300 + [b"The cat's hat isn't flat; we'll see 1234 cats.  \n" * 3, b""])
_state = {}


def models():
    """-> {"trained": learnt from the batch itself, "hand": twins on two levels, doubled spaces and the chain}"""
    if not _state:
        ids = np.random.default_rng(3).permutation(256).tolist()
        a, sp = ids[ord("a")], ids[0x20]
        hand = [(a, a, 256), (256, 256, 257), (sp, sp, 258), (258, 258, 259)] + [(ids[CHAIN[0]] if k == 0 else 259 + k, ids[CHAIN[k + 1]], 260 + k) for k in range(len(CHAIN) - 1)]
        _state.update(v=W.Vocab(["[UNK]", "a", "b"]), trained=M.train(DOCS[2:8] + DOCS[-2:], 120, seed=1), hand=M.Model(ids, hand), want={})
    return _state


def run(v, docs, tensor, slot):
    import torch
    data, off = b"".join(docs), np.cumsum([0] + [len(d) for d in docs]).astype(np.int64)
    if not tensor:
        return B.bpe_encode_rows(v, data, off, slot=slot, offsets=True, pieces=True)
    t = torch.frombuffer(bytearray(data + b"'s\xff\xff"), dtype=torch.uint8).cuda()[:len(data)]  # (dirty bytes behind the data)
    return {k: x.cpu().numpy() for k, x in B.bpe_encode_rows_tensor(v, t, torch.from_numpy(off).cuda(), slot=slot, offsets=True, pieces=True).items()}


def check(name, slot, tensor, docs=None):
    """the batch (DOCS unless given) through one form against the model: every array, and the statistics"""
    s = models()
    v, m, docs = s["v"], s[name], DOCS if docs is None else docs
    vocab, pairs = m.vocab()
    B.bpe_load(v, vocab, pairs, slot=slot)
    key = (name, len(docs))
    want = s["want"][key] = s["want"].get(key) or m.encode(docs)
    got = run(v, docs, tensor, slot)
    assert [(k, got[k].dtype) for k in got] == [("ids", np.int32), ("row_splits", np.int64), ("begin", np.int32), ("end", np.int32), ("piece_splits", np.int64)]
    for k in got:
        bad = np.flatnonzero(got[k][:len(want[k])] != want[k][:len(got[k])])[:6].tolist() if len(got[k]) and len(want[k]) else []
        assert len(got[k]) == len(want[k]) and not bad, (tensor, k, len(got[k]), len(want[k]), bad)
    lens = np.array([b - a for d in docs for a, b in M.pieces(d)] or [0])
    assert B.bpe_stats(v, slot) == dict(n_rows=len(docs), n_pieces=len(want["piece_splits"]) - 1, n_ids=len(want["ids"]), max_piece=int(lens.max()),
                                        n_short=int((lens <= SHORT).sum()) if len(want["ids"]) else 0, n_medium=int(((lens > SHORT) & (lens <= MEDIUM)).sum()),
                                        n_long=int((lens > MEDIUM).sum()), n_merges=len(m.merges), model_ids=m.n_ids, table_slots=max(16, 1 << (2 * len(m.merges) - 1).bit_length()))
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("name,tensor", [("trained", False), ("trained", True), ("hand", False), ("hand", True)])
def test_every_array_against_the_model(name, tensor):
    want = check(name, 0, tensor)
    assert len(b"".join(DOCS)) > 40 * T and len(DOCS) > 256 + 64
    if name == "hand":  # the chain ends as one id after a round per byte; the longest run of a's takes three merges in four bytes
        assert len(models()["hand"].merge(CHAIN)) == 1 and want["rounds"] == (3 * 256 + 5) * 3 // 4


@pytest.mark.gpu
def test_two_slots_survive_an_encode_and_a_trim_and_feed_the_packer():
    import torch
    from wordpiece_amd import binpack
    v, docs = models()["v"], DOCS[-3:] + [b"", b"a" * 40 + b" " + CHAIN]
    a, b = check("trained", 1, False, docs), check("hand", 2, True, docs)
    v.encode("ab a")
    W._check(W.lib().wp_trim(v._h))
    again = run(v, docs, True, 1)  # slot 1 answers as before, whatever slot 2 holds
    assert again["ids"].tolist() == a["ids"].tolist() != b["ids"].tolist() and B.bpe_stats(v, 2)["n_merges"] == len(models()["hand"].merges)
    data = torch.frombuffer(bytearray(b"".join(docs)), dtype=torch.uint8).cuda()
    r = B.bpe_encode_rows_tensor(v, data, torch.from_numpy(np.cumsum([0] + [len(d) for d in docs])).cuda(), slot=1)
    p = binpack.pack_best_fit_tensor(v, r["ids"], r["row_splits"], max_len=64, eos_id=7)
    assert sorted(r) == ["ids", "row_splits"] and int(p["lengths"].sum()) >= r["ids"].numel() > 0
    assert B.bpe_encode_rows(v, b"", [0], slot=1)["row_splits"].tolist() == [0] and B.bpe_stats(v, 1)["n_rows"] == 0  # an empty batch
    assert B.bpe_encode_docs(v, ["", ""], slot=1)["row_splits"].tolist() == [0, 0, 0]  # rows without a byte
    B.bpe_clear(v, 1)
    assert B.bpe_stats(v, 1) == dict.fromkeys(B.bpe_stats(v, 1), 0) | dict(n_rows=-1)
    with pytest.raises(W.WordPieceError, match="slot 1 holds no model"):
        B.bpe_encode_rows(v, b"a", [0, 1], slot=1)


@pytest.mark.gpu
@pytest.mark.parametrize("lib_name,guard", [("libwordpiece_amd_dbg.so", "0"), ("libwordpiece_amd.so", "1")])
def test_hardened_runs(tmp_path, lib_name, guard):
    """a fresh child on the bounds-checking build, and one under WP_ARENA_GUARD=1: no access outside an array or an arena"""
    lib = os.path.join(PKG, lib_name)
    assert os.path.exists(lib), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "bpe_hard_run.py"
    script.write_text('''
import sys
import torch  # (before the library, as tests/conftest.py: the HIP runtime loaded first serves the process)
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_bpe as T
v = T.models()["v"]
v.encode("ab a")
assert v.stats()["reserved0"] == %d, "not the build this run is about"
for name, tensor in (("trained", False), ("hand", True)):
    T.check(name, 0, tensor)
print("BPE_HARD_OK")
''' % (os.path.dirname(PKG), HERE, 1 if "dbg" in lib_name else 0))
    env = dict(os.environ, WP_LIB=lib, WP_ARENA_GUARD=guard)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "BPE_HARD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
