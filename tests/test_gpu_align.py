"""The span-alignment entry points on the GPU (wp_align, wp_align_rows and their device forms) against the Python model
(tests/align_model.py), exactly.  Most batches are synthetic offsets fed straight in, shaped where the kernels can break
(csrc/align.h): every lane-group width, a last trip that is not full, more than one trip, partial last workgroups, more
row blocks than the capped grid has workgroups, samples whose span lists end the bisection everywhere; the rest come from
the inputs and rows calls of the same handle (pairs, windows, code points, WP_OPT_NORMALIZE)."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import align_model as M
import wordpiece_amd as W

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "wordpiece_amd")
LETTERS = "abcdef"
VOCAB = ["[UNK]", "[CLS]", "[SEP]", "[PAD]"] + list(LETTERS) + ["##" + ch for ch in LETTERS] + ["ab", "##cd", "é", "##é", "中", ".", ","]
CLS, SEP, PAD = 1, 2, 3
MAX_LENS = (1, 3, 4, 5, 8, 33, 64, 65, 128, 130)
SPAN_COUNTS = (0, 1, 2, 3, 63, 64, 65)
KEYS = ("labels", "span_index", "start_positions", "end_positions")
BLOCK, MAX_GRID = 256, 2048


def test_geometry_matches_the_kernels():
    src = open(os.path.join(PKG, "csrc", "align.h")).read()
    common = open(os.path.join(PKG, "csrc", "common.h")).read()
    assert int(re.search(r"constexpr int kBlock = (\d+);", common).group(1)) == BLOCK
    assert int(re.search(r"constexpr unsigned kAlignMaxGrid = (\d+);", src).group(1)) == MAX_GRID
    assert re.search(r"kSiteAlign = 14,", common)


def _lanes(max_len):
    lanes = 4
    while lanes < 64 and lanes < max_len:
        lanes *= 2
    return lanes


def spans_for(rng, count, reach):
    """`count` sorted, disjoint, non-empty labelled spans that start below about `reach`"""
    out, p = [], rng.randint(0, 3)
    step = max(1, reach // max(count, 1))
    for _ in range(count):
        b = p + rng.randint(0, step)
        e = b + rng.randint(1, max(1, step))
        out.append((b, e, rng.randint(1, 9)))
        p = e + rng.choice((0, 0, 1, 2))
    return out


def synthetic(rng, n_rows, max_len, n_samples=None, counts=SPAN_COUNTS, pairs=True, lengths=True, identity=False):
    """offsets, types, lengths, sample of n_rows rows that look like windows of n_samples documents, and spans per sample:
    tokens ascend with gaps, specials carry (0, 0), the cells behind a row's length are dirty"""
    n_samples = n_rows if identity else (n_samples or max(1, n_rows // 2))
    offs = np.zeros((n_rows, max_len, 2), dtype=np.uint32)
    types = np.zeros((n_rows, max_len), dtype=np.int32)
    lens = np.zeros(n_rows, dtype=np.int32)
    sample = np.arange(n_rows, dtype=np.int32) if identity else np.array([rng.randrange(n_samples) for _ in range(n_rows)], dtype=np.int32)
    for r in range(n_rows):
        p = rng.choice((0, 0, 5, 40))
        turn = rng.randint(0, max_len) if pairs else max_len  # where sequence B starts
        for c in range(max_len):
            if c == turn:
                p = rng.choice((0, 7))
            types[r, c] = int(c >= turn)
            if rng.random() < 0.1:
                continue  # a special: (0, 0)
            b = p + rng.choice((0, 0, 0, 1, 2))
            e = b + rng.randint(1, 4)
            offs[r, c] = (b, e)
            p = e
        lens[r] = rng.choice((max_len, max_len, rng.randint(0, max_len)))
    reach = 3 * max_len + 40
    per_sample = [spans_for(rng, rng.choice(counts), reach) for _ in range(n_samples)]
    return dict(offsets=offs, token_type_ids=types if pairs else None, lengths=lens if lengths else None, sample=None if identity else sample), per_sample


def model(batch, per_sample, **kw):
    spec = M.Spec(batch["offsets"].shape[1], kw.get("side", 0), kw.get("outside_label", 0), kw.get("inside_add", 0), kw.get("ignore_id", -100),
                  kw.get("no_answer", 0), (1 if kw.get("labels", True) else 0) | (2 if kw.get("span_index") else 0) | (4 if kw.get("positions") else 0))
    splits, spans, labs = M.join_spans(per_sample)
    t, l, s = batch.get("token_type_ids"), batch.get("lengths"), batch.get("sample")
    res = M.align(batch["offsets"].tolist(), None if t is None else t.tolist(), None if l is None else l.tolist(), None if s is None else s.tolist(),
                  splits, spans, labs, spec)
    return M.as_arrays(res, *batch["offsets"].shape[:2]), res["stats"]


def same(got, exp, label):
    assert sorted(got) == sorted(exp), (label, sorted(got), sorted(exp))
    for k in exp:
        assert got[k].dtype == np.int32 and got[k].shape == exp[k].shape, (label, k, got[k].shape, exp[k].shape)
        bad = np.argwhere(got[k] != exp[k])
        assert len(bad) == 0, (label, k, bad[:5].tolist(), got[k][tuple(bad[0])], exp[k][tuple(bad[0])])


def check(gv, batch, per_sample, label, **kw):
    """the host entry point against the model: every wanted block and every statistic"""
    exp, stats = model(batch, per_sample, **kw)
    got = gv.align_spans(batch, per_sample, **kw)
    same(got, exp, label)
    assert gv.align_stats() == stats, (label, gv.align_stats(), stats)
    return exp, stats


ALL = dict(span_index=True, positions=True, inside_add=100, no_answer=-1)


def geometry_grid(gv):
    """every lane-group width, a last trip that is not full, more than one trip; 1, rows per workgroup - 1, that and + 1 rows"""
    rng = random.Random(41)
    n = n_cov = n_ans = 0
    for max_len in MAX_LENS:
        rpw = BLOCK // _lanes(max_len)
        for n_rows in sorted({1, rpw - 1, rpw, rpw + 1}):
            batch, per_sample = synthetic(rng, n_rows, max_len)
            for side in (0, 1):
                _, st = check(gv, batch, per_sample, ("grid", max_len, n_rows, side), side=side, **ALL)
                n_cov += st["n_covered"]
                n_ans += st["n_answer_rows"]
                n += 1
    assert n == 80 and n_cov > 2000 and n_ans > 50, (n, n_cov, n_ans)
    return n


@pytest.fixture(scope="module")
def gv():
    return W.Vocab(VOCAB)


@pytest.mark.gpu
def test_geometry_grid(gv):
    geometry_grid(gv)


@pytest.mark.gpu
def test_more_row_blocks_than_workgroups(gv):
    """max_len 4: 64 rows per workgroup, and 2049 row blocks and 3 rows for the 2048 workgroups of the capped grid: one
    workgroup runs a second block and a third, the carries start afresh and the counters add up"""
    rng = random.Random(42)
    n_rows = (MAX_GRID + 1) * (BLOCK // 4) + 3
    batch, per_sample = synthetic(rng, n_rows, 4, n_samples=500, counts=(0, 1, 2, 3))
    _, st = check(gv, batch, per_sample, "capped grid", side=0, **ALL)
    assert st["n_rows"] == n_rows and st["n_covered"] > 10000 and st["n_answer_rows"] > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("count", SPAN_COUNTS)
def test_span_counts(gv, count):
    """every sample has `count` spans: the ends of the bisection (none, one without a loop, powers of two and their neighbours)"""
    rng = random.Random(43 + count)
    batch, per_sample = synthetic(rng, 37, 70, n_samples=9, counts=(count,), pairs=False)
    exp, st = check(gv, batch, per_sample, ("count", count), **ALL)
    if count:
        assert len(np.unique(exp["span_index"])) > min(count, 20) and st["n_begin"] > 0
    else:
        assert st["n_covered"] == 0 and (exp["start_positions"] == -1).all()


def row_of(tokens, max_len):
    offs = np.zeros((1, max_len, 2), dtype=np.uint32)
    offs[0, :len(tokens)] = tokens
    return dict(offsets=offs)


@pytest.mark.gpu
def test_spans_against_token_boundaries(gv):
    toks = [(0, 0), (0, 2), (2, 5), (5, 6), (8, 10), (10, 14), (0, 0)]  # [CLS] four touching tokens, a gap, ... [SEP]
    batch = row_of(toks, 9)
    for spans, labels, index in (
            ([(5, 8, 3)], [0, 0, 3, 0, 0], [-1, -1, 0, -1, -1]),         # ends where (8, 10) begins, begins where (2, 5) ends: neither
            ([(3, 4, 3)], [0, 3, 0, 0, 0], [-1, 0, -1, -1, -1]),         # inside one token, which starts before it: the begin cell
            ([(2, 10, 3)], [0, 3, 103, 103, 0], [-1, 0, 0, 0, -1]),      # over many tokens
            ([(6, 8, 3)], [0, 0, 0, 0, 0], [-1] * 5),                    # in the blanks between tokens
            ([(14, 20, 3)], [0, 0, 0, 0, 0], [-1] * 5),                  # behind the last token
            ([(0, 3, 3), (4, 9, 4)], [3, 103, 104, 104, 0], [0, 0, 1, 1, -1]),  # (2, 5) overlaps both: the first
            ([(1, 2, 3), (2, 3, 4), (12, 13, 5)], [3, 4, 0, 0, 5], [0, 1, -1, -1, 2])):
        exp, _ = check(gv, batch, [spans], ("boundaries", spans), **ALL)
        assert exp["labels"][0].tolist() == [-100] + labels + [-100] * 3 and exp["span_index"][0].tolist() == [-1] + index + [-1] * 3, spans


def windows(n_tokens, width, stride, max_len, first=0):
    """the rows the inputs call makes of one document of n_tokens tokens (token i is the characters [2 i, 2 i + 1)): [CLS]
    window [SEP] pad, windows of `width` tokens that overlap by `stride`"""
    rows, start = [], 0
    while True:
        rows.append([(0, 0)] + [(first + 2 * i, first + 2 * i + 1) for i in range(start, min(n_tokens, start + width))] + [(0, 0)])
        if start + width >= n_tokens:
            break
        start += width - stride
    offs = np.zeros((len(rows), max_len, 2), dtype=np.uint32)
    for r, row in enumerate(rows):
        offs[r, :len(row)] = row
    return dict(offsets=offs, sample=np.zeros(len(rows), dtype=np.int32))


@pytest.mark.gpu
def test_positions_and_windows(gv):
    # 20 tokens, windows of 8 that overlap by 3: tokens 0-7, 5-12, 10-17, 15-19; column = 1 + token - first token
    batch = windows(20, 8, 3, 10)
    assert len(batch["offsets"]) == 4
    for (b, e), start, end in (((0, 1), [1, -1, -1, -1], None),                # on the first context token
                               ((38, 39), [-1, -1, -1, 5], None),             # on the last
                               ((10, 15), [6, 1, -1, -1], [8, 3, -1, -1]),    # tokens 5-7: held by two overlapping windows
                               ((14, 17), [-1, 3, -1, -1], [-1, 4, -1, -1]),  # tokens 7-8: cut by one token at the end of window 0
                               ((18, 21), [-1, 5, -1, -1], [-1, 6, -1, -1]),  # tokens 9-10: cut by one token at the start of window 2
                               ((8, 27), [-1] * 4, None),                     # tokens 4-13: held by none
                               ((11, 13), [6, 1, -1, -1], [7, 2, -1, -1])):   # begins in the blank behind token 5: start is token 5
        exp, _ = check(gv, batch, [[(b, e, 1)]], ("windows", b, e), labels=False, positions=True, no_answer=-1)
        assert exp["start_positions"].tolist() == start and exp["end_positions"].tolist() == (end or start), (b, e, exp)
    # max_len 130: the row takes three trips of 64 lanes; start and end of the answer fall in different trips
    batch = windows(128, 128, 0, 130)
    for (b, e), start, end in (((2 * 9, 2 * 99 + 1), 10, 100), ((2 * 62, 2 * 64 + 1), 63, 65), ((2 * 126, 2 * 127 + 1), 127, 128), ((0, 255), 1, 128)):
        exp, _ = check(gv, batch, [[(b, e, 1)]], ("trips", b, e), positions=True, span_index=True, no_answer=-1)
        assert (exp["start_positions"].tolist(), exp["end_positions"].tolist()) == ([start], [end])


@pytest.mark.gpu
def test_outputs_alone_and_arguments_left_out(gv):
    rng = random.Random(44)
    batch, per_sample = synthetic(rng, 45, 33, identity=True)
    for kw in (dict(labels=True), dict(labels=False, span_index=True), dict(labels=False, positions=True), dict(span_index=True),
               dict(positions=True), dict(labels=False, span_index=True, positions=True), dict(span_index=True, positions=True)):
        for side in (0, 1):
            check(gv, batch, per_sample, ("outputs", kw), side=side, inside_add=7, outside_label=2, ignore_id=-5, no_answer=-9, **kw)
    # lengths NULL, sample NULL (row r is sample r), types NULL (all 0): each alone and all together
    for drop in (("lengths",), ("sample",), ("token_type_ids",), ("lengths", "sample", "token_type_ids")):
        part, ps = synthetic(rng, 45, 33, identity="sample" in drop, n_samples=45)
        part = {k: (None if k in drop else v) for k, v in part.items()}
        check(gv, part, ps, ("dropped", drop), **ALL)


def _inputs_batch(gv, a, b, unit, **kw):
    return gv.encode_inputs(a, b, cls_id=CLS, sep_id=SEP, pad_id=PAD, offsets=unit, **kw)


@pytest.mark.gpu
def test_pairs_windows_and_code_points_from_the_inputs_call(gv):
    """question-first pairs with windows over the context, as the inputs call makes them: side 1 labels the context, side 0
    the question; code-point offsets on multi-byte text"""
    rng = random.Random(45)
    word = lambda: rng.choice(("é", "aé", "中", "ab", "abcd", "f", "cde", ".", "zz", "éé"))
    ctx = ["  ".join(word() for _ in range(rng.choice((1, 9, 30, 60)))) for _ in range(12)]
    qs = [" ".join(word() for _ in range(rng.choice((1, 3, 5)))) for _ in range(12)]
    n = 0
    for unit in ("char", "byte"):
        ulen = (lambda s: len(s)) if unit == "char" else (lambda s: len(s.encode()))
        for side, docs in ((1, ctx), (0, qs)):
            batch = _inputs_batch(gv, qs, ctx, unit, max_len=24, truncation="only_second", stride=4)
            assert len(batch["sample"]) > 12  # (windows: more rows than samples)
            per_sample = [spans_for(rng, rng.choice((0, 1, 2, 5)), ulen(d)) for d in docs]
            _, st = check(gv, batch, per_sample, ("pairs", unit, side), side=side, **ALL)
            assert st["n_covered"] > 10 and st["n_answer_rows"] + st["n_no_answer_rows"] == len(batch["sample"]), st
            n += 1
    assert n == 4


@pytest.mark.gpu
def test_normalised_hangul_shares_spans():
    """WP_OPT_NORMALIZE = 7 takes a Hangul syllable apart into jamo, and the vocabulary holds jamo pieces: the cells of one
    syllable share its source span, and the literal rule puts start behind end"""
    jamo = ["[UNK]", "[CLS]", "[SEP]", "[PAD]"] + [chr(c) for c in range(0x1100, 0x1113)] + ["##" + chr(c) for c in range(0x1100, 0x11C3)]
    gv = W.Vocab(jamo, normalize=W.WP_NORM_BERT_UNCASED)
    docs = ["한국어 각", "가 힣한", "국"]
    batch = gv.encode_inputs(docs, cls_id=CLS, sep_id=SEP, pad_id=PAD, max_len=16, offsets="char")
    offs = batch["offsets"]
    assert (offs[0, 1] == offs[0, 2]).all() and (offs[0, 2] == offs[0, 3]).all() and tuple(offs[0, 1]) == (0, 1)  # the three jamo of one syllable
    per_sample = [[(0, 1, 1), (4, 5, 2)], [(2, 4, 1)], [(0, 1, 1)]]
    exp, _ = check(gv, batch, per_sample, "hangul", **ALL)
    assert (exp["start_positions"] > exp["end_positions"]).any()
    assert exp["start_positions"][0] == 3 and exp["end_positions"][0] == 1 and exp["labels"][0, 1:4].tolist() == [1, 1, 1]


def ragged(rng, lens, counts=SPAN_COUNTS):
    rows = np.zeros(len(lens) + 1, dtype=np.int64)
    rows[1:] = np.cumsum(lens)
    offs = np.zeros((int(rows[-1]), 2), dtype=np.uint32)
    for r in range(len(lens)):
        p = 0
        for i in range(int(rows[r]), int(rows[r + 1])):
            b = p + rng.choice((0, 0, 1, 3))
            offs[i] = (b, b + rng.randint(1, 4))
            p = int(offs[i, 1])
    per_sample = [spans_for(rng, rng.choice(counts), 3 * max(int(l), 1)) for l in lens]
    return offs, rows, per_sample


def check_rows(gv, offs, rows, per_sample, label, **kw):
    splits, spans, labs = M.join_spans(per_sample)
    want = (1 if kw.get("labels", True) else 0) | (2 if kw.get("span_index") else 0)
    res = M.align_rows(offs.tolist(), rows.tolist(), splits, spans, labs, M.Spec(outside_label=kw.get("outside_label", 0), inside_add=kw.get("inside_add", 0), want=want))
    got = gv.align_rows(offs, rows, per_sample, **kw)
    exp = {k: np.array(res[k], dtype=np.int32) for k in ("labels", "span_index") if res[k] is not None}
    same(got, exp, label)
    assert gv.align_stats() == res["stats"], (label, gv.align_stats(), res["stats"])
    return exp, res["stats"]


@pytest.mark.gpu
def test_ragged_rows(gv):
    rng = random.Random(46)
    kw = dict(span_index=True, inside_add=50, outside_label=1)
    for lens in ([0, 0, 3, 5], [4, 2, 0], [0, 0, 0, 7, 0, 0, 1, 0, 0, 0], [0, 5, 0], [1], [BLOCK], [BLOCK + 1], [BLOCK - 1, 1, 1],
                 [3] * 100 + [3 * BLOCK + 17] + [2] * 100,   # one row longer than a tile (three of them) beside many short ones
                 [rng.choice((0, 1, 2, 9)) for _ in range(700)]):
        offs, rows, per_sample = ragged(rng, lens)
        _, st = check_rows(gv, offs, rows, per_sample, ("ragged", lens[:12]), **kw)
        assert st["n_tokens"] == sum(lens)
    offs, rows, per_sample = ragged(rng, [7, 0, 300, 2])
    check_rows(gv, offs, rows, per_sample, "labels alone")
    check_rows(gv, offs, rows, per_sample, "index alone", labels=False, span_index=True)


def _np(t):
    return {k: x.cpu().numpy() for k, x in t.items()}


@pytest.mark.gpu
def test_ragged_labels_into_a_packed_batch():
    """rows -> labels per id -> packed batch: one gather through `source` carries the labels, nothing leaves the device"""
    import torch
    import rows_model as R
    rng = random.Random(47)
    gv = W.Vocab(VOCAB, device=0)
    docs = [" ".join("".join(rng.choice(LETTERS) for _ in range(rng.choice((1, 2, 4)))) for _ in range(rng.choice((0, 1, 4, 12)))) for _ in range(60)]
    text, starts = R.join_docs(docs)
    t = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    ids, splits, offs = gv.encode_rows_tensor(t, torch.tensor(starts, dtype=torch.int64, device="cuda:0"), offsets="byte")
    per_sample = [spans_for(rng, rng.choice((0, 1, 3)), len(d)) for d in docs]
    lab = gv.align_rows_tensor(offs, splits, W.join_spans(per_sample), inside_add=10, span_index=True)
    assert all(x.device == ids.device and x.dtype == torch.int32 and x.shape == ids.shape for x in lab.values())
    msplits, mspans, mlabs = M.join_spans(per_sample)
    res = M.align_rows(offs.cpu().numpy().view(np.uint32).tolist(), splits.cpu().tolist(), msplits, mspans, mlabs, M.Spec(inside_add=10, want=3))
    assert lab["labels"].cpu().tolist() == res["labels"] and lab["span_index"].cpu().tolist() == res["span_index"] and res["stats"]["n_covered"] > 20
    assert gv.align_stats() == res["stats"]
    packed = gv.pack_sequences_tensor(ids, splits, max_len=16, eos_id=SEP, pad_id=PAD, want=("source",))
    src = packed["source"].long()
    carried = torch.where(src >= 0, lab["labels"][src.clamp(min=0)], torch.full_like(packed["source"], -100))
    exp = [[-100 if s < 0 else res["labels"][s] for s in row] for row in packed["source"].cpu().tolist()]
    assert carried.cpu().tolist() == exp and (carried >= 10).any()


@pytest.mark.gpu
def test_device_entry_points():
    import torch
    rng = random.Random(48)
    gv = W.Vocab(VOCAB, device=0)
    n_rows, L = 45, 100
    batch, per_sample = synthetic(rng, n_rows, L)
    exp, stats = model(batch, per_sample, side=1, **ALL)
    d = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).to("cuda:0") for k, v in batch.items()}
    sp = tuple(torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to("cuda:0") for x in W.join_spans(per_sample))
    got = gv.align_spans_tensor(d, sp, side=1, **ALL)
    assert all(x.device == d["offsets"].device and x.dtype == torch.int32 for x in got.values())
    same(_np(got), exp, "tensor")
    assert gv.align_stats() == stats
    # spans as a list: uploaded; the offsets as the uint32 view the inputs call returns
    again = gv.align_spans_tensor(dict(d, offsets=d["offsets"].view(torch.uint32)), per_sample, side=1, **ALL)
    assert all(torch.equal(got[k], again[k]) for k in got)
    # each output alone writes what all together write
    for kw, keys in ((dict(labels=True), ("labels",)), (dict(labels=False, span_index=True), ("span_index",)),
                     (dict(labels=False, positions=True), ("start_positions", "end_positions"))):
        one = gv.align_spans_tensor(d, sp, side=1, **{**ALL, "span_index": False, "positions": False, **kw})
        assert sorted(one) == sorted(keys) and all(torch.equal(one[k], got[k]) for k in keys), kw
    # nothing behind row n_rows is written, and nothing at all where the argument check of the device form fails
    cap = n_rows + 9
    big = torch.full((cap, L, 2), 3, dtype=torch.int32, device="cuda:0")
    big[:n_rows] = d["offsets"]
    outs = [torch.full((cap, L), -7, dtype=torch.int32, device="cuda:0") for _ in range(2)] + \
           [torch.full((cap,), -7, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    spec = W.AlignSpec(max_len=L, side=1, outside_label=0, inside_add=100, ignore_id=-100, no_answer=-1)
    splits, spans, labs = sp
    p = lambda x: C.c_void_p(x.data_ptr())

    def call(splits=splits, spans=spans, sample=d["sample"], n_samples=splits.numel() - 1):
        torch.cuda.synchronize()
        return W.lib().wp_align_device(gv._h, p(big), p(d["token_type_ids"]), p(d["lengths"]), p(sample), n_rows, p(splits), n_samples, p(spans),
                                       p(labs), labs.numel(), C.byref(spec), *[p(x) for x in outs])
    bad_spans = spans.clone()
    j = int(splits[1:].max()) - 1
    bad_spans[j, 1] = bad_spans[j, 0]  # the last span: empty
    bad_order = spans.clone()
    s65 = next(s for s, x in enumerate(per_sample) if len(x) >= 2)
    k = int(splits[s65]) + 1
    bad_order[k, 0] = bad_order[k - 1, 1] - 1  # begins inside the span in front of it
    bad_splits = splits.clone()
    bad_splits[3] = bad_splits[4] + 1
    bad_sample = d["sample"].clone()
    bad_sample[17] = splits.numel() - 1
    for kw, msg in ((dict(spans=bad_spans), "span %d is empty" % j), (dict(spans=bad_order), "span %d begins before span %d" % (k, k - 1)),
                    (dict(splits=bad_splits), "span_splits must start at 0, never descend and end at n_spans (entry 3)"),
                    (dict(sample=bad_sample), "the sample of row 17 is outside"), (dict(n_samples=splits.numel() - 2), "align: ")):
        assert call(**kw) == 6 and msg in W.lib().wp_last_error().decode(), (msg, W.lib().wp_last_error())
        assert all(bool((x == -7).all()) for x in outs), msg
    assert call() == 0
    for x, k in zip(outs, KEYS):
        assert torch.equal(x[:n_rows], got[k]) and bool((x[n_rows:] == -7).all()), k
    assert bool((big[n_rows:] == 3).all()) and gv.align_stats() == stats
    # the ragged device form: the same check, the same silence; n_ids must be the last entry of row_splits
    offs, rows, ps = ragged(rng, [0, 5, 0, 0, BLOCK + 40, 3, 0])
    d_offs, d_rows = torch.from_numpy(offs.view(np.int32)).to("cuda:0"), torch.from_numpy(rows).to("cuda:0")
    r_splits, r_spans, r_labs = (torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to("cuda:0") for x in W.join_spans(ps))
    n = offs.shape[0]
    o2 = [torch.full((n + 50,), -7, dtype=torch.int32, device="cuda:0") for _ in range(2)]

    def call_rows(rows=d_rows, n_ids=n, spans=r_spans):
        torch.cuda.synchronize()
        return W.lib().wp_align_rows_device(gv._h, p(d_offs), p(rows), rows.numel() - 1, n_ids, p(r_splits), p(spans) if spans.numel() else None,
                                            p(r_labs) if r_labs.numel() else None, r_labs.numel(), C.byref(spec), p(o2[0]), p(o2[1]))
    bad_rows = d_rows.clone()
    bad_rows[2] = bad_rows[1] - 1
    for kw, msg in ((dict(rows=bad_rows), "row_splits must start at 0, never descend and end at n_ids (entry 1)"), (dict(n_ids=n - 1), "row_splits must")):
        assert call_rows(**kw) == 6 and msg in W.lib().wp_last_error().decode(), (msg, W.lib().wp_last_error())
        assert all(bool((x == -7).all()) for x in o2), msg
    assert call_rows() == 0
    t = gv.align_rows_tensor(d_offs, d_rows, (r_splits, r_spans, r_labs), inside_add=100, span_index=True)
    assert torch.equal(o2[0][:n], t["labels"]) and torch.equal(o2[1][:n], t["span_index"]) and all(bool((x[n:] == -7).all()) for x in o2)
    exp_rows, st_rows = check_rows(gv, offs, rows, ps, "ragged host", inside_add=100, span_index=True)
    assert np.array_equal(t["labels"].cpu().numpy(), exp_rows["labels"]) and np.array_equal(t["span_index"].cpu().numpy(), exp_rows["span_index"])
    # an encode on this handle is what it was, and says so in the statistics
    assert gv.encode("ab a").tolist() == [VOCAB.index("ab"), VOCAB.index("a")] and gv.align_stats()["n_rows"] == -1


@pytest.mark.gpu
def test_sizes_up_and_down_around_trim(gv):
    rng = random.Random(49)
    for n_rows, max_len, trim in ((3, 8, False), (400, 130, False), (2, 5, True), (300, 64, False), (1, 1, True), (50, 33, False)):
        if trim:
            gv.trim()
        batch, per_sample = synthetic(rng, n_rows, max_len)
        check(gv, batch, per_sample, ("sizes", n_rows, max_len, trim), side=rng.randint(0, 1), **ALL)
        offs, rows, ps = ragged(rng, [rng.choice((0, 3, 40)) for _ in range(n_rows)])
        check_rows(gv, offs, rows, ps, ("sizes ragged", n_rows, trim), span_index=True)


@pytest.mark.gpu
def test_bounds_checking_build(tmp_path):
    """(child on the bounds-checking build with WP_ARENA_GUARD=1) the grid and a ragged batch: no sample outside the splits,
    no gather outside the span list (kSiteAlign), no guard zone of the host call's arena overwritten"""
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    script = tmp_path / "align_dbg_run.py"
    script.write_text('''
import random, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import wordpiece_amd as W
from test_gpu_align import VOCAB, BLOCK, geometry_grid, ragged, check_rows
gv = W.Vocab(VOCAB)
gv.encode("ab a")
assert gv.stats()["reserved0"] == 1, "not the bounds-checking build"
assert geometry_grid(gv) == 80
rng = random.Random(50)
offs, rows, ps = ragged(rng, [0, 4, 0, 2 * BLOCK + 9, 1] + [2] * 300)
check_rows(gv, offs, rows, ps, "debug ragged", span_index=True, inside_add=5)
print("ALIGN_DEBUG_OK")
''' % (os.path.dirname(PKG), HERE))
    env = dict(os.environ, WP_LIB=dbg, WP_ARENA_GUARD="1")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "ALIGN_DEBUG_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
