"""The masking entry points on the GPU (wp_mlm_mask, wp_word_ids and their device forms) against the Python model
(tests/mask_model.py), bit for bit.  The id batches are synthetic numpy arrays fed straight in; the shapes sit where
the kernel can break — every lane-group width, more than one trip of the column loop, partial last workgroups whose
idle lane groups share a wave with live ones — not at workload size."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import mask_model as M
import wordpiece_amd as W

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")
LETTERS = "abcdefghijklmnopqrstuvwxyz"
VOCAB = ["[UNK]", "[CLS]", "[SEP]", "[PAD]", "[MASK]"] + list(LETTERS) + ["##" + ch for ch in LETTERS] + [".."]
UNK, CLS, SEP, PAD, MASK = 0, 1, 2, 3, 4
V = len(VOCAB)
FLAGS = M.flags_of(VOCAB)
WORD, CONT, BAD = 5, 5 + 26, V - 1  # "a", "##a", the malformed line
MAX_LENS = (1, 3, 4, 5, 8, 31, 32, 33, 63, 64, 65, 128, 129, 200)
BASE = M.Spec(max_len=0, cls_id=CLS, sep_id=SEP, pad_id=PAD, mask_id=MASK, ignore_id=-100, whole_word=1, select_q32=M.q32(0.15),
              mask_q32=M.q32(0.8), random_q32=M.q32(0.1), seed=0, row_base=0)


def _lanes(max_len):
    lanes = 4
    while lanes < 64 and lanes < max_len:
        lanes *= 2
    return lanes


def _batch(rng, n_rows, max_len):
    from test_mask_model import random_batch
    ids, lengths = random_batch(rng, n_rows, max_len, V, FLAGS, (CLS, SEP, PAD))
    return np.array(ids, dtype=np.int64).astype(np.int32).reshape(n_rows, max_len), None if lengths is None else np.array(lengths, dtype=np.int32)


def _kw(spec):
    return dict(mask_id=spec.mask_id, whole_word=bool(spec.whole_word), seed=spec.seed, row_base=spec.row_base, ignore_id=spec.ignore_id,
                cls_id=spec.cls_id, sep_id=spec.sep_id, pad_id=spec.pad_id)


def _call(gv, ids, lengths, spec, word_ids=True):
    """the host entry point with the spec's q32 values (the Python mirror takes shares: set them on the struct)"""
    cs = W._mask_spec(ids.shape[1], spec.mask_id, 0.0, 0.0, 0.0, spec.whole_word, spec.seed, spec.row_base, spec.ignore_id, spec.cls_id,
                      spec.sep_id, spec.pad_id)
    cs.select_q32, cs.mask_q32, cs.random_q32 = spec.select_q32, spec.mask_q32, spec.random_q32
    i32p = C.POINTER(C.c_int32)
    masked, labels, wids = i32p(), i32p(), i32p()
    W._check(W.lib().wp_mlm_mask(gv._h, W._i32_ptr(ids), W._i32_ptr(lengths), ids.shape[0], C.byref(cs), C.byref(masked), C.byref(labels),
                                 C.byref(wids) if word_ids else None))
    res = {"input_ids": W._adopt_block(masked, ids.shape), "labels": W._adopt_block(labels, ids.shape)}
    if word_ids:
        res["word_ids"] = W._adopt_block(wids, ids.shape)
    return res


def _same(got, exp, shape, label, keys=("input_ids", "labels", "word_ids")):
    for k in keys:
        assert got[k].dtype == np.int32 and got[k].shape == shape, (label, k)
        assert np.array_equal(got[k], np.array(exp[k], dtype=np.int64).reshape(shape)), (label, k)


def _check(gv, ids, lengths, spec, label=None):
    spec = spec._replace(max_len=ids.shape[1])
    exp = M.mask(FLAGS, ids.tolist(), None if lengths is None else lengths.tolist(), spec)
    got = _call(gv, ids, lengths, spec)
    _same(got, exp, ids.shape, (label, spec))
    assert gv.mask_stats() == exp["stats"], (label, spec, gv.mask_stats(), exp["stats"])
    return exp


def geometry_grid(gv):
    """every lane-group width and more than one trip; 1, rows per workgroup - 1, that, + 1 and 3 x + 2 rows; both units"""
    rng = random.Random(21)
    n = n_sel = 0
    for max_len in MAX_LENS:
        rpw = 256 // _lanes(max_len)
        for n_rows in (1, rpw - 1, rpw, rpw + 1, 3 * rpw + 2):
            ids, lengths = _batch(rng, n_rows, max_len)
            for whole_word in (1, 0):
                exp = _check(gv, ids, lengths, BASE._replace(whole_word=whole_word, select_q32=M.q32(0.4), seed=rng.getrandbits(64),
                                                             row_base=rng.choice((0, 2 ** 40))), "grid")
                n_sel += exp["stats"]["n_selected"]
                n += 1
    assert n == 140 and n_sel > 10000
    return n


@pytest.fixture(scope="module")
def handle():
    return W.Vocab(VOCAB)


@pytest.mark.gpu
def test_geometry_grid(handle):
    geometry_grid(handle)


@pytest.mark.gpu
def test_more_row_blocks_than_workgroups(handle):
    """the grid is capped at 2048 workgroups, which then take several row blocks each: 2050 blocks of 4 rows (3 rows in the
    last), so that two workgroups run a second block — the carries start afresh and the counters add up"""
    rng = random.Random(25)
    n_rows, max_len = 2049 * 4 + 3, 33
    ids, _ = _batch(rng, n_rows, max_len)
    lengths = np.array([rng.randint(0, max_len) for _ in range(n_rows)], dtype=np.int32)
    exp = _check(handle, ids, lengths, BASE._replace(select_q32=M.q32(0.3), seed=4), "capped grid")
    assert exp["stats"]["n_selected"] > 20000 and any(map(any, exp["selected"][8192:]))


def _constructed():
    L = 200
    rows, lengths = [], []

    def add(row, length=L):
        assert len(row) == L
        rows.append(row)
        lengths.append(length)

    add([CLS] + [WORD + 1] * 61 + [WORD, CONT] + [CONT + 1] * 63 + [CONT + 2, CONT + 3] + [WORD + 2] * 70 + [SEP])  # words over 63|64, 127|128
    add([CONT + i % 26 for i in range(L)])                    # one word of 200 ## tokens
    add([WORD] + [CONT + i % 26 for i in range(L - 1)])       # the same behind a word start
    add([(CLS, SEP, PAD)[i % 3] for i in range(L)])           # all specials
    add([WORD + i % 5 for i in range(L)], 0)                  # lengths 0
    add([WORD, CONT] * (L // 2), L)                           # lengths max_len
    add([WORD] * 63 + [SEP] + [CONT] * (L - 64))              # [SEP] at 63, ## at 64
    add([WORD] * 63 + [UNK] + [CONT] * (L - 64))              # [UNK] at 63, ## at 64
    add([WORD] * 63 + [BAD] + [CONT] * 63 + [V] + [CONT] * (L - 128))  # malformed at 63; out of range at 127, ## at 128
    add([CONT] * 64 + [-1] + [CONT] * 62 + [2 ** 31 - 1] + [CONT] * (L - 128), 150)
    return np.array(rows, dtype=np.int64).astype(np.int32), np.array(lengths, dtype=np.int32)


@pytest.mark.gpu
def test_constructed_rows(handle):
    ids, lengths = _constructed()
    for whole_word in (1, 0):
        for seed in (1, 2):
            spec = BASE._replace(whole_word=whole_word, select_q32=M.q32(0.5), seed=seed)
            exp = _check(handle, ids, lengths, spec, "constructed")
            wid = exp["word_ids"]
            assert wid[0][61:130] == [60] + [61] * 67 + [62] and wid[1] == [0] * 200 and wid[2] == [0] * 200 and set(wid[3]) == {-1} == set(wid[4])
            assert wid[6][63:66] == [-1, 0, 0] and wid[7][62:66] == [62, 63, 64, 64] and wid[8][126:130] == [64, -1, 0, 0]
            if whole_word:  # a word of 200 tokens is selected as one
                assert len(set(exp["selected"][1])) == 1 and len(set(exp["selected"][0][62:129])) == 1
    # lengths NULL against lengths given: rows whose length is max_len anyway
    full = np.flatnonzero(lengths == 200)
    a = _call(handle, ids[full], None, BASE._replace(max_len=200, seed=9))
    b = _call(handle, ids[full], lengths[full], BASE._replace(max_len=200, seed=9))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    _check(handle, ids, None, BASE._replace(seed=9), "no lengths")


@pytest.mark.gpu
def test_probability_edges(handle):
    rng = random.Random(22)
    ids, _ = _batch(rng, 37, 70)
    lengths = np.array([rng.randint(35, 70) for _ in range(37)], dtype=np.int32)
    for whole_word in (1, 0):
        spec = BASE._replace(whole_word=whole_word, seed=5)
        exp = _check(handle, ids, lengths, spec._replace(select_q32=0), "select 0")
        assert exp["stats"]["n_selected"] == 0 and exp["input_ids"] == ids.tolist()
        exp = _check(handle, ids, lengths, spec._replace(select_q32=M.ONE), "select all")
        assert exp["stats"]["n_selected"] > 1000
        exp = _check(handle, ids, lengths, spec._replace(select_q32=M.ONE, mask_q32=M.ONE, random_q32=0), "mask all")
        assert exp["stats"]["n_masked"] == exp["stats"]["n_selected"] > 1000
        exp = _check(handle, ids, lengths, spec._replace(select_q32=M.ONE, mask_q32=0, random_q32=M.ONE), "random all")
        assert exp["stats"]["n_random"] == exp["stats"]["n_selected"] > 1000
        picked = [y for row, sel in zip(exp["input_ids"], exp["selected"]) for y, s in zip(row, sel) if s]
        assert min(picked) >= 0 and max(picked) < V and len(set(picked)) > V // 2
        exp = _check(handle, ids, lengths, spec._replace(select_q32=M.ONE, mask_q32=0, random_q32=0, ignore_id=7), "keep all")
        assert exp["stats"]["n_kept"] == exp["stats"]["n_selected"] and exp["input_ids"] == ids.tolist()
    # the Python mirror's shares are the q32 values the model takes
    got = handle.mask_inputs(ids, lengths, prob=0.3, mask_share=0.5, random_share=0.25, word_ids=True, **_kw(BASE._replace(seed=3)))
    exp = M.mask(FLAGS, ids.tolist(), lengths.tolist(), BASE._replace(max_len=70, seed=3, select_q32=M.q32(0.3), mask_q32=M.q32(0.5),
                                                                       random_q32=M.q32(0.25)))
    _same(got, exp, ids.shape, "shares")
    assert sorted(handle.mask_inputs(ids, lengths, mask_id=MASK)) == ["input_ids", "labels"]


def _np(t):
    return {k: x.cpu().numpy() for k, x in t.items()}


@pytest.mark.gpu
def test_device_entry_points():
    import torch
    rng = random.Random(23)
    gv = W.Vocab(VOCAB, device=0)
    n_rows, L = 45, 100
    ids, lengths = _batch(rng, n_rows, L)
    lengths = np.array([rng.randint(0, L) for _ in range(n_rows)], dtype=np.int32)
    spec = BASE._replace(max_len=L, seed=77, select_q32=M.q32(0.3))
    kw = dict(prob=0.3, **_kw(spec))
    exp = M.mask(FLAGS, ids.tolist(), lengths.tolist(), spec)
    d_ids, d_len = torch.from_numpy(ids).to("cuda:0"), torch.from_numpy(lengths).to("cuda:0")
    got = gv.mask_inputs_tensor(d_ids, d_len, word_ids=True, **kw)
    assert all(x.device == d_ids.device and x.dtype == torch.int32 for x in got.values()) and got["input_ids"].data_ptr() != d_ids.data_ptr()
    _same(_np(got), exp, ids.shape, "tensor")
    assert gv.mask_stats() == exp["stats"] and np.array_equal(d_ids.cpu().numpy(), ids)
    # the same seed: the same batch; another seed: another
    again = gv.mask_inputs_tensor(d_ids, d_len, word_ids=True, **kw)
    assert all(torch.equal(got[k], again[k]) for k in got)
    other = gv.mask_inputs_tensor(d_ids, d_len, **dict(kw, seed=78))
    assert not torch.equal(other["labels"], got["labels"]) and sorted(other) == ["input_ids", "labels"]
    # without word ids: the same masked ids and labels
    plain = gv.mask_inputs_tensor(d_ids, d_len, **kw)
    assert torch.equal(plain["input_ids"], got["input_ids"]) and torch.equal(plain["labels"], got["labels"])
    # the word-ids call on its own
    wid = gv.word_ids_tensor(d_ids, d_len, cls_id=CLS, sep_id=SEP, pad_id=PAD)
    assert torch.equal(wid, got["word_ids"])
    st = gv.mask_stats()
    assert st == dict(exp["stats"], n_selected=0, n_selected_units=0, n_masked=0, n_random=0, n_kept=0, whole_word=0)
    assert np.array_equal(gv.word_ids(ids, lengths, cls_id=CLS, sep_id=SEP, pad_id=PAD), np.array(exp["word_ids"]))
    # slices of one buffer with row_base are the rows of the whole batch
    for a, b in ((0, 7), (7, 8), (8, 45), (44, 45), (13, 13)):
        part = gv.mask_inputs_tensor(d_ids[a:b], d_len[a:b], word_ids=True, **dict(kw, row_base=a))
        assert all(torch.equal(part[k], got[k][a:b]) for k in got), (a, b)
    # in place equals out of place
    work = d_ids.clone()
    inp = gv.mask_inputs_tensor(work, d_len, in_place=True, **kw)
    assert inp["input_ids"].data_ptr() == work.data_ptr() and torch.equal(work, got["input_ids"]) and torch.equal(inp["labels"], got["labels"])
    # nothing behind row n_rows is written: buffers of 9 more rows, filled with a sentinel
    cap = n_rows + 9
    big_in = torch.full((cap, L), -7, dtype=torch.int32, device="cuda:0")
    big_in[:n_rows] = d_ids
    outs = [torch.full((cap, L), -7, dtype=torch.int32, device="cuda:0") for _ in range(3)]
    cs = W._mask_spec(L, **{k: v for k, v in dict(kw, mask_share=0.8, random_share=0.1).items()})
    torch.cuda.synchronize()
    W._check(W.lib().wp_mlm_mask_device(gv._h, C.c_void_p(big_in.data_ptr()), C.c_void_p(d_len.data_ptr()), n_rows, C.byref(cs),
                                        *[C.c_void_p(x.data_ptr()) for x in outs]))
    for x, k in zip(outs, ("input_ids", "labels", "word_ids")):
        assert torch.equal(x[:n_rows], got[k]) and bool((x[n_rows:] == -7).all()), k
    assert bool((big_in[n_rows:] == -7).all())
    # a handle on which nothing else ran gives the same, and an encode on this one is what it was
    assert all(torch.equal(W.Vocab(VOCAB, device=0).mask_inputs_tensor(d_ids, d_len, word_ids=True, **kw)[k], got[k]) for k in got)
    assert gv.encode("abc a").tolist() == [WORD, CONT + 1, CONT + 2, WORD] and gv.mask_stats()["n_rows"] == -1


@pytest.mark.gpu
def test_composition_with_the_inputs_call():
    """encode_inputs_tensor (pairs, windows with stride) -> mask_inputs_tensor on the returned device tensors is the model
    applied to the model's batch"""
    import torch
    import inputs_model as I
    import rows_model as R
    rng = random.Random(24)
    gv, model = W.Vocab(VOCAB, device=0), R.Model(VOCAB)
    word = lambda: "".join(rng.choice(LETTERS[:6]) for _ in range(rng.choice((1, 1, 2, 3, 5)))) if rng.random() < 0.93 else "?!"
    docs = [" ".join(word() for _ in range(rng.choice((0, 1, 3, 8, 20)))).encode() for _ in range(2 * 40)]
    text, starts = R.join_docs(docs)
    t = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    d_off = torch.tensor(starts, dtype=torch.int64, device="cuda:0")
    n = 0
    for ispec, name, stride in ((I.Spec(24, CLS, SEP, PAD, 1), "longest_first", None), (I.Spec(24, CLS, SEP, PAD, 1, I.ONLY_SECOND, 5), "only_second", 5),
                                (I.Spec(9, CLS, SEP, PAD, 0, I.ONLY_FIRST, 2), "only_first", 2)):
        batch = I.build(model, docs, ispec)
        got = gv.encode_inputs_tensor(t, d_off, pairs=bool(ispec.pairs), max_len=ispec.max_len, cls_id=CLS, sep_id=SEP, pad_id=PAD,
                                      truncation=name, stride=stride, n_out=len(batch["lengths"]))
        assert np.array_equal(got["input_ids"].cpu().numpy(), np.array(batch["input_ids"]))
        spec = BASE._replace(max_len=ispec.max_len, seed=n, select_q32=M.q32(0.25))
        for lengths in (batch["lengths"], None):  # the dict's lengths, or the pad id alone
            exp = M.mask(FLAGS, batch["input_ids"], lengths, spec)
            src = got if lengths is not None else got["input_ids"]
            res = gv.mask_inputs_tensor(src, word_ids=True, prob=0.25, **_kw(spec))
            _same(_np(res), exp, (len(batch["lengths"]), ispec.max_len), ("composition", ispec))
            assert gv.mask_stats() == exp["stats"] and exp["stats"]["n_selected"] > 20
        n += 1
    assert n == 3


@pytest.mark.gpu
def test_bounds_checking_build(tmp_path):
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "mask_dbg_run.py"
    script.write_text('''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import wordpiece_amd as W
from test_gpu_mask import VOCAB, geometry_grid
gv = W.Vocab(VOCAB)
gv.encode("abc a")
assert gv.stats()["reserved0"] == 1, "not the bounds-checking build"
assert geometry_grid(gv) == 140
print("MASK_DEBUG_OK")
''' % (os.path.dirname(PKG), HERE))
    env = dict(os.environ, WP_LIB=dbg)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "MASK_DEBUG_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
