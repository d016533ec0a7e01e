"""CPU checks of the masking entry points (wp_mlm_mask, wp_word_ids, their device forms, wp_get_mask_stats): the structs
against the header, what the calls answer without a device — argument errors, empty batches — and that anything else
fails loudly without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import wordpiece_amd as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = ["[UNK]", "[MASK]", "a", "##b"]
ARG, TOO_LARGE = 6, 2


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


def test_structs_match_the_header(tmp_path):
    widths = {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint64_t": C.c_uint64}
    for name, mirror in (("wp_mask_spec", W.MaskSpec), ("wp_mask_stats", W.MaskStats)):
        assert [(n, widths[t]) for n, t in _header_fields(name)] == list(mirror._fields_), name
    assert [f[0] for f in W.MaskStats._fields_] == ["n_rows", "n_words", "n_selected", "n_selected_units", "n_masked", "n_random", "n_kept",
                                                    "whole_word", "reserved"]
    assert [f[0] for f in W.Stats._fields_][-1] == "rows_route"  # wp_stats keeps its size and its end
    probes = [("wp_mask_spec", f[0], W.MaskSpec) for f in W.MaskSpec._fields_] + [("wp_mask_stats", f[0], W.MaskStats) for f in W.MaskStats._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu\\n", sizeof(wp_stats), sizeof(wp_mask_spec), sizeof(wp_mask_stats));\n' +
                   "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (s, f) for s, f, _ in probes) + "  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:3] == [C.sizeof(W.Stats), C.sizeof(W.MaskSpec), C.sizeof(W.MaskStats)] == [C.sizeof(W.Stats), 72, 64]
    assert got[3:] == [getattr(m, f).offset for _, f, m in probes]
    for name in ("wp_word_ids", "wp_word_ids_device", "wp_mlm_mask", "wp_mlm_mask_device", "wp_get_mask_stats"):
        assert name in W.ABI_SYMBOLS and hasattr(W.lib(), name)


def _spec(**kw):
    s = W.MaskSpec(max_len=4, cls_id=-1, sep_id=-1, pad_id=-1, mask_id=1, ignore_id=-100, whole_word=1, select_q32=W.q32(0.15),
                   mask_q32=W.q32(0.8), random_q32=W.q32(0.1))
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_argument_errors_come_before_the_device():
    L = W.lib()
    v = W.Vocab(VOCAB)
    ids = np.array([[2, 3, 2, 0]] * 2, dtype=np.int32)
    p_ids = W._i32_ptr(ids)
    i32p = C.POINTER(C.c_int32)
    masked, labels, wids = i32p(), i32p(), i32p()
    dev = C.c_void_p(256)  # (never dereferenced: the argument rules come first)

    def calls(spec, n_rows=2, mask_only=False):
        sp = None if spec is None else C.byref(spec)
        out = [("wp_mlm_mask", lambda: L.wp_mlm_mask(v._h, p_ids, None, n_rows, sp, C.byref(masked), C.byref(labels), C.byref(wids))),
               ("wp_mlm_mask_device", lambda: L.wp_mlm_mask_device(v._h, dev, None, n_rows, sp, dev, dev, None))]
        if not mask_only:
            out += [("wp_word_ids", lambda: L.wp_word_ids(v._h, p_ids, None, n_rows, sp, C.byref(wids))),
                    ("wp_word_ids_device", lambda: L.wp_word_ids_device(v._h, dev, None, n_rows, sp, dev))]
        return out

    big = 2 ** 32 + 1
    for spec, msg, mask_only, code in ((None, b"spec is NULL", False, ARG), (_spec(max_len=0), b"max_len", False, ARG),
                                       (_spec(max_len=-3), b"max_len", False, ARG), (_spec(whole_word=2), b"whole_word", True, ARG),
                                       (_spec(whole_word=-1), b"whole_word", True, ARG), (_spec(select_q32=big), b"select_q32", True, ARG),
                                       (_spec(mask_q32=big, random_q32=0), b"mask_q32", True, ARG),
                                       (_spec(mask_q32=0, random_q32=big), b"random_q32", True, ARG),
                                       (_spec(mask_q32=2 ** 31 + 1, random_q32=2 ** 31), b"mask_q32 + random_q32", True, ARG),
                                       (_spec(mask_id=-1), b"mask_id", True, ARG)):
        for n_rows in (2, 0):  # (and for a batch that needs no device)
            for name, call in calls(spec, n_rows, mask_only):
                rc = call()
                assert rc == code and msg in L.wp_last_error(), (name, msg, rc, L.wp_last_error())
                assert not masked and not labels and not wids
    # the word-ids calls read max_len and the three specials only
    assert L.wp_word_ids(v._h, p_ids, None, 0, C.byref(_spec(whole_word=9, select_q32=big, mask_id=-1)), C.byref(wids)) == 0
    # sizes (with 64-bit sizes the row limit comes first: INT32_MAX rows of INT32_MAX int32 cells are still addressable)
    for n_rows, max_len in ((2 ** 31, 1), (2 ** 40, 2 ** 31 - 1)):
        for name, call in calls(_spec(max_len=max_len), n_rows):
            rc = call()
            assert rc == TOO_LARGE and b"mask: " in L.wp_last_error(), (name, rc, L.wp_last_error())
    # NULL pointers, by name
    sp = C.byref(_spec())
    for call, msg in ((lambda: L.wp_mlm_mask(v._h, None, None, 2, sp, C.byref(masked), C.byref(labels), None), b"input_ids"),
                    (lambda: L.wp_mlm_mask(v._h, p_ids, None, 2, sp, None, C.byref(labels), None), b"masked"),
                    (lambda: L.wp_mlm_mask(v._h, p_ids, None, 2, sp, C.byref(masked), None, None), b"labels"),
                    (lambda: L.wp_word_ids(v._h, None, None, 2, sp, C.byref(wids)), b"input_ids"),
                    (lambda: L.wp_word_ids(v._h, p_ids, None, 2, sp, None), b"word_ids"),
                    (lambda: L.wp_mlm_mask_device(v._h, None, None, 2, sp, dev, dev, None), b"input_ids"),
                    (lambda: L.wp_mlm_mask_device(v._h, dev, None, 2, sp, None, dev, None), b"masked"),
                    (lambda: L.wp_mlm_mask_device(v._h, dev, None, 2, sp, dev, None, None), b"labels"),
                    (lambda: L.wp_word_ids_device(v._h, None, None, 2, sp, dev), b"input_ids"),
                    (lambda: L.wp_word_ids_device(v._h, dev, None, 2, sp, None), b"word_ids")):
        rc = call()
        assert rc == ARG and msg + b" is NULL" in L.wp_last_error(), (msg, rc, L.wp_last_error())
    # the Python mirror's own rules
    with pytest.raises(W.WordPieceError, match="mask_id is required"):
        v.mask_inputs(ids)
    with pytest.raises(W.WordPieceError, match="prob must lie"):
        v.mask_inputs(ids, mask_id=1, prob=1.5)
    with pytest.raises(W.WordPieceError, match="mask_q32 . random_q32"):
        v.mask_inputs(ids, mask_id=1, mask_share=0.8, random_share=0.3)
    with pytest.raises(W.WordPieceError, match="2-d"):
        v.mask_inputs(ids[0], mask_id=1)
    with pytest.raises(W.WordPieceError, match="n_rows entries"):
        v.word_ids(ids, lengths=[1, 2, 3])
    assert W.q32(0.0) == 0 and W.q32(1.0) == 2 ** 32 and W.q32(0.15) == int(0.15 * 2 ** 32) and W.q32(1e-12) == 0


def test_empty_batches_need_no_device():
    v = W.Vocab(VOCAB)
    assert v.mask_stats()["n_rows"] == -1  # a fresh handle: no mask call yet
    out = v.mask_inputs(np.zeros((0, 7), dtype=np.int32), mask_id=1, word_ids=True, whole_word=False)
    assert sorted(out) == ["input_ids", "labels", "word_ids"] and all(x.shape == (0, 7) and x.dtype == np.int32 for x in out.values())
    assert v.mask_stats() == dict(n_rows=0, n_words=0, n_selected=0, n_selected_units=0, n_masked=0, n_random=0, n_kept=0, whole_word=0)
    assert sorted(v.mask_inputs(np.zeros((0, 7), dtype=np.int32), mask_id=1)) == ["input_ids", "labels"]
    assert v.mask_stats()["whole_word"] == 1
    assert v.word_ids(np.zeros((0, 3), dtype=np.int32)).shape == (0, 3) and v.mask_stats()["n_rows"] == 0
    # through the C ABI: NULL blocks, and the device forms accept NULL buffers for no rows
    L = W.lib()
    i32p = C.POINTER(C.c_int32)
    masked, labels, wids = i32p(), i32p(), i32p()
    sp = C.byref(W.MaskSpec(max_len=3, mask_id=1, whole_word=1))
    assert L.wp_mlm_mask(v._h, None, None, 0, sp, C.byref(masked), C.byref(labels), C.byref(wids)) == 0
    assert not masked and not labels and not wids
    assert L.wp_mlm_mask_device(v._h, None, None, 0, sp, None, None, None) == 0
    assert L.wp_word_ids_device(v._h, None, None, 0, sp, None) == 0


def test_no_cpu_fallback_for_masking():
    if W.lib().wp_device_count() > 0:
        pytest.skip("GPU present")
    v = W.Vocab(VOCAB)
    ids = np.array([[2, 3, 2, 0]], dtype=np.int32)
    for call in (lambda: v.mask_inputs(ids, mask_id=1), lambda: v.mask_inputs(ids, lengths=[2], mask_id=1, word_ids=True),
                 lambda: v.word_ids(ids)):
        with pytest.raises(W.WordPieceError, match="no HIP device"):
            call()
    L = W.lib()
    dev = C.c_void_p(256)
    sp = C.byref(W.MaskSpec(max_len=4, mask_id=1, whole_word=1))
    assert L.wp_mlm_mask_device(v._h, dev, None, 1, sp, dev, dev, None) == 4 and b"no HIP device" in L.wp_last_error()  # WP_ERR_NO_DEVICE
    assert L.wp_word_ids_device(v._h, dev, None, 1, sp, dev) == 4 and b"no HIP device" in L.wp_last_error()
