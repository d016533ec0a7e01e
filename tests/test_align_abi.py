"""CPU checks of the span-alignment entry points (wp_align, wp_align_rows, their device forms, wp_get_align_stats): the
structs against the header, what the host entry points answer without a device — every argument error, with the first
offender named as tests/align_model.py names it, and batches without a row — and that anything else fails loudly without
a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import align_model as M
import wordpiece_amd as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = ["[UNK]", "a", "##b"]
ARG, TOO_LARGE, NO_DEVICE = 6, 2, 4
SYMBOLS = ("wp_align", "wp_align_device", "wp_align_rows", "wp_align_rows_device", "wp_get_align_stats")


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(W.LIB_PATH):
        from wordpiece_amd import build
        build.build()


def _header_fields(name):
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd.h")).read()
    end = hdr.index("} %s;" % name)
    body = hdr[hdr.rindex("typedef struct {", 0, end):end]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("typedef struct {", "")
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


def test_symbols_and_structs_match_the_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in W.ABI_SYMBOLS and hasattr(W.lib(), name), name
    widths = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    mirrors = (("wp_align_spec", W.AlignSpec), ("wp_align_stats", W.AlignStats))
    for name, mirror in mirrors:
        assert [(n, widths[t]) for n, t in _header_fields(name)] == list(mirror._fields_), name
    assert [f[0] for f in W.AlignSpec._fields_] == ["max_len", "side", "outside_label", "inside_add", "ignore_id", "no_answer", "want", "reserved"]
    assert [f[0] for f in W.AlignStats._fields_] == ["n_rows", "n_tokens", "n_covered", "n_begin", "n_spans", "n_answer_rows", "n_no_answer_rows"]
    probes = [(name, f[0], m) for name, m in mirrors for f in m._fields_]
    others = ("wp_stats", "wp_mask_stats", "wp_detok_stats", "wp_pack_stats", "wp_special_stats", "wp_inputs_stats")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu\\n", sizeof(wp_align_spec), sizeof(wp_align_stats));\n'
                   '  printf("%d %d %d\\n", WP_ALIGN_LABELS, WP_ALIGN_SPAN_INDEX, WP_ALIGN_POSITIONS);\n' +
                   "".join('  printf("%%zu\\n", sizeof(%s));\n' % s for s in others) +
                   "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (s, f) for s, f, _ in probes) + "  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:2] == [C.sizeof(W.AlignSpec), C.sizeof(W.AlignStats)] == [32, 56]
    assert got[2:5] == [W.WP_ALIGN_LABELS, W.WP_ALIGN_SPAN_INDEX, W.WP_ALIGN_POSITIONS] == [M.LABELS, M.SPAN_INDEX, M.POSITIONS] == [1, 2, 4]
    # the other statistics structs keep their sizes
    assert got[5:11] == [C.sizeof(W.Stats), C.sizeof(W.MaskStats), C.sizeof(W.DetokStats), C.sizeof(W.PackStats), C.sizeof(W.SpecialStats),
                         C.sizeof(W.InputsStats)] == [C.sizeof(W.Stats), 64, 48, 64, 32, 48]
    assert got[11:] == [getattr(m, f).offset for _, f, m in probes]


def _spec(**kw):
    s = W.AlignSpec(max_len=2, side=0, outside_label=0, inside_add=1, ignore_id=-100, no_answer=0, want=7)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


OFFSETS = np.array([[[0, 1], [1, 2]], [[0, 2], [0, 0]]], dtype=np.uint32)  # 2 rows of 2 cells
GOOD = ([0, 1, 2], [(0, 1), (1, 2)], [1, 2])


def _host(v, spec, splits=GOOD[0], spans=GOOD[1], labs=GOOD[2], offsets=OFFSETS, types=None, lengths=None, sample=None, n_rows=None, outs=None):
    """wp_align on host arrays -> (rc, the four out blocks as addresses)"""
    i32p, u32p = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    s = None if splits is None else np.ascontiguousarray(splits, dtype=np.int64)
    sp = None if spans is None else np.ascontiguousarray(spans, dtype=np.uint32).reshape(-1, 2)
    sl = None if labs is None else np.ascontiguousarray(labs, dtype=np.int32)
    arr = [None if x is None else np.ascontiguousarray(x, dtype=np.int32) for x in (types, lengths, sample)]
    blocks = [i32p() for _ in range(4)] if outs is None else outs
    rc = W.lib().wp_align(v._h, None if offsets is None else offsets.ctypes.data_as(u32p), *[W._i32_ptr(x) for x in arr],
                          len(offsets) if n_rows is None else n_rows, W._i64_ptr(s), 0 if s is None else len(s) - 1,
                          None if sp is None else sp.ctypes.data_as(u32p), W._i32_ptr(sl), 0 if sp is None else len(sp),
                          None if spec is None else C.byref(spec), *[None if b is None else C.byref(b) for b in blocks])
    return rc, [None if b is None else C.cast(b, C.c_void_p).value for b in blocks]


def _model_message(splits, spans, n_rows=2, sample=None, row_splits=None, n_ids=None):
    with pytest.raises(ValueError) as e:
        M.check_arrays(splits, spans, n_rows, sample, row_splits, n_ids)
    return str(e.value).encode()


def test_argument_errors_come_before_the_device():
    L = W.lib()
    v = W.Vocab(VOCAB)
    assert v.align_stats()["n_rows"] == -1  # a fresh handle: no align call yet
    types = np.zeros((2, 2), dtype=np.int32)
    dev = C.c_void_p(256)  # (never dereferenced: the argument rules come first)

    def device(spec, types=None, labels=dev, index=dev, start=dev, end=dev, offsets=dev, span_labels=dev, n_rows=2, n_samples=2, n_spans=2):
        return L.wp_align_device(v._h, offsets, types, None, None, n_rows, dev, n_samples, dev, span_labels, n_spans,
                                 None if spec is None else C.byref(spec), labels, index, start, end)

    # the spec, in both forms
    for spec, kw, msg in ((None, {}, b"spec is NULL"), (_spec(max_len=0), {}, b"max_len must be at least 1"), (_spec(max_len=-3), {}, b"max_len must be at least 1"),
                          (_spec(side=2), dict(types=types), b"side must be 0 or 1"), (_spec(side=-1), dict(types=types), b"side must be 0 or 1"),
                          (_spec(side=1), {}, b"side 1 needs token_type_ids")):
        rc, blocks = _host(v, spec, **kw)
        assert rc == ARG and msg in L.wp_last_error() and not any(blocks), (msg, rc, L.wp_last_error())
        assert device(spec, types=dev if kw else None) == ARG and msg in L.wp_last_error(), (msg, L.wp_last_error())
    # want (host form); the device form names its outputs by their pointers
    for spec, kw, msg in ((_spec(want=0), {}, b"no output is wanted"), (_spec(want=8), {}, b"bits outside 7"), (_spec(want=-1), {}, b"bits outside 7"),
                          (_spec(want=1), dict(labs=None), b"labels wanted without span_labels"),
                          (_spec(want=7), dict(labs=None), b"labels wanted without span_labels")):
        rc, blocks = _host(v, spec, **kw)
        assert rc == ARG and msg in L.wp_last_error() and not any(blocks), (msg, rc, L.wp_last_error())
    assert device(_spec(), labels=None, index=None, start=None, end=None) == ARG and b"no output is wanted" in L.wp_last_error()
    assert device(_spec(), start=None) == ARG and b"go together" in L.wp_last_error()
    assert device(_spec(), span_labels=None) == ARG and b"labels wanted without span_labels" in L.wp_last_error()
    # pointers
    i32p = C.POINTER(C.c_int32)
    for call, msg in ((lambda: _host(v, _spec(), splits=None)[0], b"span_splits is NULL"),
                      (lambda: _host(v, _spec(), offsets=None, n_rows=2)[0], b"offsets is NULL"),
                      (lambda: _host(v, _spec(want=1), outs=[None, i32p(), i32p(), i32p()])[0], b"out-pointer of a wanted output"),
                      (lambda: _host(v, _spec(want=4), outs=[i32p(), i32p(), i32p(), None])[0], b"out-pointer of a wanted output"),
                      (lambda: device(_spec(), offsets=None), b"offsets is NULL"),
                      (lambda: device(_spec(), offsets=C.c_void_p(260)), b"8-byte aligned"),
                      (lambda: device(_spec(), labels=C.c_void_p(258)), b"4-byte aligned"),
                      (lambda: device(_spec(), types=C.c_void_p(257)), b"4-byte aligned")):
        rc = call()
        assert rc == ARG and msg in L.wp_last_error(), (msg, rc, L.wp_last_error())
    # an unwanted output may be NULL in the host call
    if L.wp_device_count() == 0:
        assert _host(v, _spec(want=2), labs=None, outs=[None, i32p(), None, None])[0] == NO_DEVICE
    # the arrays, each with the first offender named as the model names it
    for splits, spans, name in ((GOOD[0], [(0, 1), (2, 2)], b"span 1 is empty"), (GOOD[0], [(1, 1), (2, 2)], b"span 0 is empty"),
                                (GOOD[0], [(5, 2), (0, 1)], b"span 0 is empty"),
                                ([0, 2, 2], [(3, 4), (1, 2)], b"span 1 begins before span 0"),            # unsorted
                                ([0, 2, 2], [(0, 3), (2, 4)], b"span 1 begins before span 0"),            # overlapping
                                ([0, 0, 3], [(0, 1), (1, 2), (1, 3)], b"span 2 begins before span 1"),
                                ([0, 3, 3], [(0, 1), (0, 0), (0, 3)], b"span 1 is empty"),                # the first of two offenders
                                ([1, 1, 2], GOOD[1], b"span_splits must start at 0"), ([0, 2, 1], GOOD[1], b"entry 1"),
                                ([0, 1, 3], GOOD[1], b"entry 2"), ([0, 1, 1], GOOD[1], b"entry 2"), ([0, -1, 2], GOOD[1], b"entry 0")):
        rc, blocks = _host(v, _spec(), splits=splits, spans=spans, labs=[1] * len(spans))
        assert rc == ARG and name in L.wp_last_error() and not any(blocks), (splits, spans, L.wp_last_error())
        assert L.wp_last_error() == _model_message(splits, spans), (splits, spans)
    # spans of different samples are not held against each other
    if L.wp_device_count() == 0:
        assert _host(v, _spec(), spans=[(3, 4), (1, 2)])[0] == NO_DEVICE
    for sample, n_rows, name in (([0, 2], 2, b"row 1"), ([-1, 0], 2, b"row 0"), ([2, 5], 2, b"row 0")):
        rc, blocks = _host(v, _spec(), sample=sample)
        assert rc == ARG and b"the sample of " + name in L.wp_last_error() and not any(blocks), sample
        assert L.wp_last_error() == _model_message(GOOD[0], GOOD[1], n_rows, sample)
    rc, blocks = _host(v, _spec(), splits=[0, 2], sample=None)  # sample NULL: row r is sample r, and there is one sample
    assert rc == ARG and b"the sample of row 1" in L.wp_last_error() and not any(blocks)
    # the ragged form
    u32p = C.POINTER(C.c_uint32)
    flat = np.array([[0, 1], [1, 2], [0, 2]], dtype=np.uint32)

    def rows(spec, row_splits, splits=GOOD[0], spans=GOOD[1], labs=GOOD[2]):
        r, s = np.array(row_splits, dtype=np.int64), np.array(splits, dtype=np.int64)
        sp, sl = np.array(spans, dtype=np.uint32).reshape(-1, 2), np.array(labs, dtype=np.int32)
        a, b = i32p(), i32p()
        rc = L.wp_align_rows(v._h, flat.ctypes.data_as(u32p), W._i64_ptr(r), len(r) - 1, W._i64_ptr(s), sp.ctypes.data_as(u32p), W._i32_ptr(sl),
                             len(sp), None if spec is None else C.byref(spec), C.byref(a), C.byref(b))
        return rc, bool(a) or bool(b)
    for spec, row_splits, kw, msg in ((None, [0, 1, 3], {}, b"spec is NULL"), (_spec(want=4), [0, 1, 3], {}, b"the ragged form has no positions"),
                                      (_spec(want=7), [0, 1, 3], {}, b"the ragged form has no positions"), (_spec(want=0), [0, 1, 3], {}, b"no output"),
                                      (_spec(want=3), [1, 1, 3], {}, b"row_splits must start at 0"), (_spec(want=3), [0, 2, 1], {}, b"row_splits must"),
                                      (_spec(want=3), [0, 1, -3], {}, b"row_splits must"),
                                      (_spec(want=3), [0, 1, 3], dict(spans=[(0, 1), (4, 4)]), b"span 1 is empty"),
                                      (_spec(want=3), [0, 1, 3], dict(splits=[0, 1, 1]), b"span_splits must")):
        rc, any_block = rows(spec, row_splits, **kw)
        assert rc == ARG and msg in L.wp_last_error() and not any_block, (msg, L.wp_last_error())
    if L.wp_device_count() == 0:
        assert rows(_spec(want=3, max_len=0, side=9), [0, 1, 3])[0] == NO_DEVICE  # max_len and side are not read: the rules pass
    rc = L.wp_align_rows_device(v._h, dev, None, 2, 3, dev, dev, dev, 2, C.byref(_spec()), dev, dev)
    assert rc == ARG and b"row_splits is NULL" in L.wp_last_error()
    rc = L.wp_align_rows_device(v._h, dev, C.c_void_p(260), 2, 3, dev, dev, dev, 2, C.byref(_spec()), dev, dev)
    assert rc == ARG and b"8-byte aligned" in L.wp_last_error()
    rc = L.wp_align_rows_device(v._h, dev, dev, 2, 3, dev, dev, dev, 2, C.byref(_spec()), None, None)
    assert rc == ARG and b"no output is wanted" in L.wp_last_error()
    # sizes: nothing is dereferenced behind what the rule needs
    for kw, msg in ((dict(n_rows=2 ** 31), b"more rows"), (dict(n_samples=2 ** 31), b"more samples"), (dict(n_spans=2 ** 31), b"more spans")):
        assert device(_spec(), **kw) == TOO_LARGE and msg in L.wp_last_error(), msg
    assert device(_spec(max_len=2 ** 31 - 1), n_rows=2 ** 31 - 1) == TOO_LARGE and b"n_rows * max_len" in L.wp_last_error()  # 2^62 cells of 8 B
    assert L.wp_align_rows_device(v._h, dev, dev, 2, 2 ** 31, dev, dev, dev, 2, C.byref(_spec()), dev, dev) == TOO_LARGE and b"more ids" in L.wp_last_error()
    # the Python mirror's own rules
    with pytest.raises(W.WordPieceError, match="needs an output"):
        v.align_spans(offsets=OFFSETS, spans=[[], []], labels=False)
    with pytest.raises(W.WordPieceError, match="needs the offsets"):
        v.align_spans({"input_ids": np.zeros((2, 2), np.int32)}, [[], []])
    with pytest.raises(W.WordPieceError, match="one list of spans per row"):
        v.align_rows(flat, [0, 1, 3], [[]])
    with pytest.raises(W.WordPieceError, match="span 0 is empty"):
        v.align_spans(offsets=OFFSETS, spans=[[(3, 3)], []])
    if L.wp_device_count() == 0:
        assert v.align_stats()["n_rows"] == -1  # none of this was a call


def test_batches_without_rows_need_no_device():
    v = W.Vocab(VOCAB)
    empty = np.zeros((0, 5, 2), dtype=np.uint32)
    out = v.align_spans(offsets=empty, spans=[[(0, 3, 1)], []], span_index=True, positions=True)
    assert sorted(out) == ["end_positions", "labels", "span_index", "start_positions"]
    assert out["labels"].shape == out["span_index"].shape == (0, 5) and out["start_positions"].shape == out["end_positions"].shape == (0,)
    exp = M.align([], None, None, None, [0, 1, 1], [(0, 3)], [1], M.Spec(5, want=7))["stats"]
    assert v.align_stats() == exp == dict(n_rows=0, n_tokens=0, n_covered=0, n_begin=0, n_spans=1, n_answer_rows=0, n_no_answer_rows=0)
    rc, blocks = _host(v, _spec(), offsets=None, n_rows=0)  # through the C ABI: NULL blocks; offsets may be NULL where there are no rows
    assert rc == 0 and not any(blocks)
    # the argument rules hold for a batch without rows too
    rc, blocks = _host(v, _spec(), offsets=None, n_rows=0, spans=[(0, 1), (1, 1)])
    assert rc == ARG and b"span 1 is empty" in W.lib().wp_last_error()
    # ragged: rows without ids
    for splits in ([0], [0, 0], [0, 0, 0, 0]):
        out = v.align_rows(np.zeros((0, 2), np.uint32), splits, [[(1, 2, 3)]] * (len(splits) - 1), span_index=True)
        assert out["labels"].shape == out["span_index"].shape == (0,)
        assert v.align_stats() == dict(n_rows=len(splits) - 1, n_tokens=0, n_covered=0, n_begin=0, n_spans=len(splits) - 1, n_answer_rows=0,
                                       n_no_answer_rows=0)


def test_join_spans():
    splits, spans, labs = W.join_spans([[(1, 2, 3)], [], [(4, 5), (6, 9, 1)]])
    assert splits.dtype == np.int64 and spans.dtype == np.uint32 and labs.dtype == np.int32
    assert splits.tolist() == [0, 1, 1, 3] and spans.tolist() == [[1, 2], [4, 5], [6, 9]] and labs.tolist() == [3, 0, 1]
    assert tuple(x.tolist() for x in W.join_spans([])) == ([0], [], []) and W.join_spans([])[1].shape == (0, 2)
    ms, mp, ml = M.join_spans([[(1, 2, 3)], [], [(4, 5), (6, 9, 1)]])
    assert (ms, [list(p) for p in mp], ml) == (splits.tolist(), spans.tolist(), labs.tolist())


def test_no_cpu_fallback_for_alignment():
    if W.lib().wp_device_count() > 0:
        pytest.skip("GPU present")
    v = W.Vocab(VOCAB)
    with pytest.raises(W.WordPieceError, match="no HIP device"):
        v.align_spans(offsets=OFFSETS, spans=[[(0, 1, 1)], []])
    with pytest.raises(W.WordPieceError, match="no HIP device"):
        v.align_rows(OFFSETS.reshape(-1, 2), [0, 2, 4], [[(0, 1, 1)], []])
    dev = C.c_void_p(256)
    rc = W.lib().wp_align_device(v._h, dev, None, None, None, 2, dev, 2, dev, dev, 2, C.byref(_spec()), dev, None, None, None)
    assert rc == NO_DEVICE and b"no HIP device" in W.lib().wp_last_error()
    rc = W.lib().wp_align_rows_device(v._h, dev, dev, 2, 3, dev, dev, dev, 2, C.byref(_spec()), dev, dev)
    assert rc == NO_DEVICE and b"no HIP device" in W.lib().wp_last_error()
