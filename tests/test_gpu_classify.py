"""GPU checks of the classifier against tests/classify_model.py: every array of both forms, over models drawn from a seeded
generator and one batch of documents built around the kernels' sizes (csrc/classify.h): the byte tile T of the token and
feature passes, the 64-byte groups of the feature prefix, the units of 4 * lanes-per-row features of the accumulation (4,
64 and 256 features at dim 1, 16 and 50 / 64), and one batch of many blocks of the accumulation at dim 1."""
import os
import subprocess
import sys

import numpy as np
import pytest

import classify_model as M
import wordpiece_amd as W
from wordpiece_amd import classify as K

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")
T, TABLE = K.TILE_BYTES, 32  # TABLE: the dictionary slots of 9..16 words (classify_path.h, classify_table)
sp = lambda n: b" " * n  # noqa: E731
CHARS = "aé€\U0001f600b".encode()  # characters of 1, 2, 3, 4 and 1 bytes
CLASH = [w for w in (b"w%d" % k for k in range(400)) if M.H(w) % TABLE == M.H(b"w0") % TABLE][:3]  # one home slot: two words and a token that is none
WORDS = [b"a", b"abc", b"def", b"ghij", CHARS[1:6], b"\xff\xfe", b"</s>", b"a", CLASH[0], CLASH[1], b"h", b"q" * 40]
DOCS = ([b"a " * 192, b"a " * 64, b"a a a"]  # 256 word features: a document boundary on the edge of every unit size
        + [sp(T - 517 - 3) + b"abc",b"def" + sp(T - 5) + b"ghij" + sp(T - 2)]  # a token up to the last byte of tile 0, from the first of tile 1, over the next edge
        + [sp(T - s) + CHARS + sp(T + s - len(CHARS)) for s in range(1, len(CHARS))]  # every character of CHARS over a tile edge, at each of its bytes
        + [b"\x80\x80a\xc3 \xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbf\xbfz \xff\xfe \xff",
           b"a\x00b\tc\x0bd\x0ce\rf\ng h", b"", b"   \n", b"", b"x </s> y", b"</s>", b"</s>x <", b" ".join(CLASH), b"q" * (T + 50) + b" a", sp(64 - 9) + b"h"]
        + [b"h"] * 300 + [b"abc def " * k for k in (2, 4, 8, 20)] + [b""])
_handle = []


def handle():
    if not _handle:
        _handle.append(W.Vocab(["[UNK]", "a", "b"]))
    return _handle[0]


def draw(seed, dim, n_labels, minn, maxn, N, bucket, exact=True, eos=True):
    """a model of the words above: the reference and what classify_load takes"""
    rng = np.random.default_rng(seed)
    words = [w for w in WORDS if eos or w != b"</s>"]
    shape = (len(words) + bucket, dim), (n_labels, dim)
    inp, outp = (rng.integers(-16, 17, s) / 8.0 for s in shape) if exact else (rng.standard_normal(s) for s in shape)
    if exact and dim == 1:  # (one column: sums that cannot be 0 and output rows that differ, or the logits tie)
        inp, outp = np.abs(inp) + 0.125 * (inp == 0), (rng.permutation(33)[:n_labels].reshape(-1, 1) - 16) / 8.0
    inp, outp = inp.astype(np.float32), outp.astype(np.float32)
    return M.Model(words, inp, outp, minn, maxn, N, bucket), dict(words=words, input=inp, output=outp, minn=minn, maxn=maxn, word_ngrams=N, bucket=bucket)


def run(v, docs, tensor, **how):
    import torch
    data, off = b"".join(docs), np.cumsum([0] + [len(d) for d in docs]).astype(np.int64)
    if not tensor:
        return K.classify_rows(v, data, off, logits=True, compact=True, raw=True, **how)
    t = torch.frombuffer(bytearray(data + b"z\xff\xff\xff"), dtype=torch.uint8).cuda()[:len(data)]  # (dirty bytes behind the data)
    got = {k: x.cpu().numpy() for k, x in K.classify_rows_tensor(v, t, torch.from_numpy(off).cuda(), logits=True, compact=True, **how).items()}
    assert got["reasons"].dtype == np.int32
    return dict(got, reasons=got["reasons"].view(np.uint32))


def check_exact(seed, dim, n_labels, minn, maxn, N, bucket, eos=True, slot=0, batch=None):
    """the batch (DOCS unless given), with every document of more than 256 features blanked, through both forms against the model"""
    v = handle()
    for attempt in range(40):  # the reference alone decides: distinct top-two logits in every document, no probability at the bound of min_prob
        ref, args = draw(seed + 1000 * attempt, dim, n_labels, minn, maxn, N, bucket, eos=eos)
        docs = [d if len(ref.features(d)[0]) <= 256 else sp(len(d)) for d in batch or DOCS]
        keep, rel = list(range(0, n_labels, 2)), (n_labels + 4) * 2.0 ** -23
        plain = [ref.score(d) for d in docs]
        ps = np.unique([p["prob"] for p in plain if p["F"]])
        gaps = [k for k in range(len(ps) - 1) if ps[k + 1] - ps[k] > 8 * rel * ps[k + 1]]  # min_prob in the middle of a gap near the median, 0 where there is none
        min_prob = float(np.float32((ps[gaps[len(gaps) // 2]] + ps[gaps[len(gaps) // 2] + 1]) / 2)) if gaps else 0.0
        if all(p["F"] == 0 or n_labels == 1 or np.diff(np.sort(p["logits"])[-2:])[0] > 0 for p in plain) and all(abs(p["prob"] - min_prob) > 2 * rel * p["prob"] + 1e-12 for p in plain):
            break
    else:
        raise AssertionError("no seed gives the reference its margins")
    exp = [ref.score(d, keep, min_prob) for d in docs]
    assert sum(p["F"] > 64 for p in exp) >= 1 and sum(p["F"] == 0 for p in exp) >= (0 if eos else 3) and len({p["reasons"] for p in exp}) >= min(2, n_labels)
    K.classify_load(v, slot=slot, **args)
    for tensor in (False, True):
        got = run(v, docs, tensor, slot=slot, keep_labels=keep, min_prob=min_prob)
        assert [(k, got[k].dtype) for k in got] == [("label", np.int32), ("prob", np.float32), ("n_features", np.int64), ("reasons", np.uint32), ("logits", np.float32),
                                                    ("kept", np.int32), ("data", np.uint8), ("row_off", np.int64)] and got["logits"].shape == (len(docs), n_labels)
        for key, name in (("n_features", "F"), ("label", "label"), ("reasons", "reasons")):
            bad = [(r, int(got[key][r]), p[name]) for r, p in enumerate(exp) if got[key][r] != p[name]][:6]
            assert not bad, (tensor, key, bad)
        want = np.array([np.float32(p["logits"]) for p in exp])  # (S and the products are exact: float32(exact / F))
        assert np.all(np.abs(got["logits"] - want) <= 2 * np.spacing(np.abs(want))), (tensor, np.argwhere(np.abs(got["logits"] - want) > 2 * np.spacing(np.abs(want)))[:6])
        prob = np.array([p["prob"] for p in exp])
        assert np.all(np.abs(got["prob"] - prob) <= rel * prob), (tensor, np.argwhere(np.abs(got["prob"] - prob) > rel * prob)[:6])
        kept = [r for r, p in enumerate(exp) if p["reasons"] == 0]
        assert got["kept"].tolist() == kept and got["data"].tobytes() == b"".join(docs[r] for r in kept) and got["row_off"].tolist() == np.cumsum([0] + [len(docs[r]) for r in kept]).tolist()
        feats = [ref.features(d) for d in docs]
        assert K.classify_stats(v, slot) == dict(n_rows=len(docs), n_kept=len(kept), n_features=sum(len(f[0]) for f in feats), n_tokens=sum(f[1] for f in feats), n_found=sum(f[2] for f in feats),
                                                 n_words=len(args["words"]), bucket=bucket, dim=dim, n_labels=n_labels, minn=minn, maxn=maxn, word_ngrams=N)
    return docs, exp


SHAPES = [(16, 176, 0, 0, 1, 1, True), (1, 1, 1, 1, 1, 7, True), (16, 65, 2, 4, 1, 2 ** 20, True), (50, 2, 3, 6, 1, 7, False), (64, 2, 0, 0, 2, 2 ** 20, True), (16, 2, 0, 0, 5, 1, False),
          (64, 65, 2, 4, 2, 7, True), (50, 176, 1, 1, 5, 2 ** 20, False), (1, 2, 3, 6, 2, 1, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("dim,n_labels,minn,maxn,N,bucket,eos", SHAPES, ids=["dim%d-L%d-n%d.%d-N%d-B%d-eos%d" % s for s in SHAPES])
def test_exact_models_against_the_reference(dim, n_labels, minn, maxn, N, bucket, eos):
    docs, exp = check_exact(7, dim, n_labels, minn, maxn, N, bucket, eos)
    assert len(b"".join(docs)) > 20 * T and (maxn > 0 or N > 1 or exp[0]["F"] >= 192)  # (words alone: the first two documents fill 256 features to the edge of a unit)


@pytest.mark.gpu
def test_many_blocks_of_the_accumulation():
    """dim 1: a unit is 4 features and a workgroup takes 256 units, so 160 documents of 100 to 253 word features fill over 20 workgroups"""
    docs, exp = check_exact(13, 1, 2, 0, 0, 1, 1, batch=[b"a " * (100 + r % 150) + b"h " * (r % 5) for r in range(160)])
    assert sum(p["F"] for p in exp) > 20 * 256 * K.UNIT_STEPS and max(p["F"] for p in exp) <= 256


@pytest.mark.gpu
def test_a_real_valued_model_within_the_forward_error_bound():
    v, (ref, args) = handle(), draw(11, 100, 176, 2, 4, 1, 5003, exact=False)
    docs = [d for d in DOCS if len(d) < 4 * T] + [b"the quick brown fox " * 200]
    K.classify_load(v, slot=0, **args)
    got, again = run(v, docs, True), run(v, docs, True)
    assert all(np.array_equal(got[k], again[k]) for k in got)  # the same bits in every run
    skipped = 0
    for r, d in enumerate(docs):
        f, p = ref.features(d)[0], ref.score(d)
        assert got["n_features"][r] == len(f)
        if not f:
            continue
        bound = (len(f) + 100 + 2) * 2.0 ** -24 * (np.abs(ref.outp) @ np.abs(ref.inp[f].astype(np.float64)).sum(axis=0)) / len(f)
        assert np.all(np.abs(got["logits"][r] - p["logits"]) <= bound), r
        top = np.argsort(p["logits"])[-2:]
        if p["logits"][top[1]] - p["logits"][top[0]] > 2 * bound[top].max():
            assert got["label"][r] == p["label"], r
        else:
            skipped += 1
    assert skipped <= len(docs) // 100


@pytest.mark.gpu
def test_slots_survive_encodes_and_trim_and_feed_the_dedup():
    import torch
    v = handle()
    docs, a = check_exact(3, 16, 2, 0, 0, 1, 1, slot=1)
    _, b = check_exact(5, 16, 65, 2, 4, 1, 7, slot=2)
    v.encode("ab a")
    W._check(W.lib().wp_trim(v._h))
    got = run(v, docs, False, slot=1)  # slot 1 answers as before, whatever slot 2 holds
    assert got["label"].tolist() == [p["label"] for p in a] and K.classify_stats(v, 2)["n_labels"] == 65 and [p["F"] for p in a] != [p["F"] for p in b]
    t = torch.frombuffer(bytearray(b"".join(docs)), dtype=torch.uint8).cuda()
    r = K.classify_rows_tensor(v, t, torch.from_numpy(np.cumsum([0] + [len(d) for d in docs])).cuda(), slot=1, compact=True)
    d = v.dedup_rows_tensor(r["data"], r["row_off"])
    assert len(d["first"]) == len(r["kept"]) and len(set(docs[k] for k in r["kept"].tolist())) == len(d["kept"])
    keep = np.array([0, 2], dtype=np.int32)  # a keep label outside the model is an argument error, in both forms
    with pytest.raises(W.WordPieceError, match=r"classify: keep_labels\[1\] is no label"):
        K.classify_rows(v, b"a", [0, 1], slot=1, keep_labels=keep)
    with pytest.raises(W.WordPieceError, match=r"classify: keep_labels\[1\] is no label"):
        K.classify_rows_tensor(v, t[:4], torch.tensor([0, 4], dtype=torch.int64).cuda(), slot=1, keep_labels=keep)
    assert K.classify_rows(v, b"", [0], slot=1, compact=True)["row_off"].tolist() == [0] and K.classify_stats(v, 1)["n_rows"] == 0  # an empty batch
    assert K.classify_docs(v, ["a a", ""], slot=1, compact=True)["docs"] == [b"a a", b""]
    K.classify_clear(v, 1)
    assert K.classify_stats(v, 1) == dict.fromkeys(K.classify_stats(v, 1), 0) | dict(n_rows=-1)
    with pytest.raises(W.WordPieceError, match="slot 1 holds no model"):
        K.classify_rows(v, b"a", [0, 1], slot=1)


@pytest.mark.gpu
@pytest.mark.parametrize("lib_name,guard", [("libwordpiece_amd_dbg.so", "0"), ("libwordpiece_amd.so", "1")])
def test_hardened_runs(tmp_path, lib_name, guard):
    """a fresh child on the bounds-checking build, and one under WP_ARENA_GUARD=1: no access outside an array or an arena"""
    lib = os.path.join(PKG, lib_name)
    assert os.path.exists(lib), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "classify_hard_run.py"
    script.write_text('''
import sys
import torch  # (before the library, as tests/conftest.py: the HIP runtime loaded first serves the process)
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_classify as T
v = T.handle()
v.encode("ab a")
assert v.stats()["reserved0"] == %d, "not the build this run is about"
for shape in (T.SHAPES[0], T.SHAPES[2], T.SHAPES[6]):
    T.check_exact(7, *shape)
print("CLASSIFY_HARD_OK")
''' % (os.path.dirname(PKG), HERE, 1 if "dbg" in lib_name else 0))
    env = dict(os.environ, WP_LIB=lib, WP_ARENA_GUARD=guard)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "CLASSIFY_HARD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
