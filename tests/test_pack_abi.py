"""CPU checks of the pack entry points (wp_pack_sequences, its device form, wp_get_pack_stats): the structs against the
header, what the host entry point answers without a device — argument and size errors, batches without a row — and that
anything else fails loudly without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pack_model as M
import wordpiece_amd as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = ["[UNK]", "a", "##b"]
ARG, TOO_LARGE = 6, 2
I32_MAX = 2 ** 31 - 1


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
            fields += [(n.strip().lstrip("*"), ctype if "*" not in n else "ptr") for n in names.split(",")]
    return fields


def test_structs_match_the_header(tmp_path):
    widths = {"int64_t": C.c_int64, "int32_t": C.c_int32, "ptr": C.c_void_p}
    mirrors = (("wp_pack_spec", W.PackSpec), ("wp_packed", W.Packed), ("wp_pack_stats", W.PackStats))
    for name, mirror in mirrors:
        assert [(n, widths[t]) for n, t in _header_fields(name)] == list(mirror._fields_), name
    assert [f[0] for f in W.Stats._fields_][-1] == "rows_route"  # wp_stats keeps its size and its end
    probes = [(name, f[0], m) for name, m in mirrors for f in m._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(wp_stats), sizeof(wp_pack_spec), sizeof(wp_packed), sizeof(wp_pack_stats));\n'
                   '  printf("%d %d %d %d %d %d %d\\n", WP_PACK_NEXT_FIT, WP_PACK_STREAM, WP_PACK_LONG_TRUNCATE, WP_PACK_LONG_SPLIT,\n'
                   '         WP_PACK_WANT_SEGMENTS, WP_PACK_WANT_POSITIONS, WP_PACK_WANT_SOURCE);\n' +
                   "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (s, f) for s, f, _ in probes) + "  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:4] == [C.sizeof(W.Stats), C.sizeof(W.PackSpec), C.sizeof(W.Packed), C.sizeof(W.PackStats)] == \
        [C.sizeof(W.Stats), 32, 5 * C.sizeof(C.c_void_p), 64]
    assert got[4:11] == [W.WP_PACK_NEXT_FIT, W.WP_PACK_STREAM, W.WP_PACK_LONG_TRUNCATE, W.WP_PACK_LONG_SPLIT,
                         W.WP_PACK_WANT_SEGMENTS, W.WP_PACK_WANT_POSITIONS, W.WP_PACK_WANT_SOURCE] == [0, 1, 0, 1, 1, 2, 4]
    assert (M.NEXT_FIT, M.STREAM, M.LONG_TRUNCATE, M.LONG_SPLIT) == (0, 1, 0, 1)
    assert got[11:] == [getattr(m, f).offset for _, f, m in probes]
    for name in ("wp_pack_sequences", "wp_pack_sequences_device", "wp_get_pack_stats"):
        assert name in W.ABI_SYMBOLS and hasattr(W.lib(), name)


def _spec(**kw):
    s = W.PackSpec(max_len=4, mode=0, bos_id=-1, eos_id=-1, pad_id=0, long_docs=0, want=7)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _host(v, ids, splits, spec, out=None, n=None):
    out = W.Packed() if out is None else out
    n = C.c_size_t(77) if n is None else n
    a = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
    s = None if splits is None else np.ascontiguousarray(splits, dtype=np.int64)
    rc = W.lib().wp_pack_sequences(v._h, W._i32_ptr(a), W._i64_ptr(s), 0 if s is None else len(s) - 1,
                                   None if spec is None else C.byref(spec), C.byref(out), C.byref(n))
    return rc, out, n.value


def _blocks(out):
    return [out.input_ids, out.segment_ids, out.position_ids, out.source, out.lengths]


def test_argument_errors_come_before_the_device():
    L = W.lib()
    v = W.Vocab(VOCAB)
    assert v.pack_stats()["n_docs"] == -1  # a fresh handle: no pack call yet
    ids, splits = [1, 2, 1], [0, 2, 3]
    dev = C.c_void_p(256)  # (never dereferenced: the argument rules come first)
    bufs = W.Packed(256, 256, 256, 256, 256)
    n = C.c_size_t()
    for spec, msg in ((None, b"spec is NULL"), (_spec(mode=2), b"unknown mode"), (_spec(mode=-1), b"unknown mode"),
                      (_spec(long_docs=2), b"long_docs"), (_spec(long_docs=-1), b"long_docs"), (_spec(want=8), b"want"),
                      (_spec(want=-1), b"want"), (_spec(max_len=0), b"max_len"), (_spec(max_len=-4), b"max_len"),
                      (_spec(max_len=1, eos_id=5), b"no room"), (_spec(max_len=2, bos_id=0, eos_id=5), b"no room")):
        rc, out, rows = _host(v, ids, splits, spec)
        assert rc == ARG and msg in L.wp_last_error() and rows == 0 and not any(_blocks(out)), (msg, rc, L.wp_last_error())
        rc = L.wp_pack_sequences_device(v._h, dev, dev, 2, None if spec is None else C.byref(spec), C.byref(bufs), 8, C.byref(n))
        assert rc == ARG and msg in L.wp_last_error(), (msg, rc, L.wp_last_error())
    # long_docs is not read in stream mode
    assert _host(v, [], [0, 0], _spec(mode=1, long_docs=9))[0] == 0
    # pointers
    sp = _spec()
    for call, msg in ((lambda: _host(v, ids, None, sp)[0], b"row_splits is NULL"), (lambda: _host(v, None, splits, sp)[0], b"ids is NULL"),
                      (lambda: L.wp_pack_sequences(v._h, None, None, 0, C.byref(sp), None, C.byref(n)), b"out-pointer"),
                      (lambda: L.wp_pack_sequences(v._h, None, None, 0, C.byref(sp), C.byref(bufs), None), b"out-pointer"),
                      (lambda: L.wp_pack_sequences_device(v._h, dev, None, 2, C.byref(sp), C.byref(bufs), 8, C.byref(n)), b"row_splits is NULL"),
                      (lambda: L.wp_pack_sequences_device(v._h, dev, dev, 2, C.byref(sp), None, 8, C.byref(n)), b"out-pointer"),
                      (lambda: L.wp_pack_sequences_device(v._h, dev, dev, 2, C.byref(sp), C.byref(bufs), 8, None), b"out-pointer"),
                      (lambda: L.wp_pack_sequences_device(v._h, dev, dev, 2, C.byref(sp), C.byref(W.Packed(256, 256, 256, None, 256)), 8,
                                                          C.byref(n)), b"output buffer is NULL"),
                      (lambda: L.wp_pack_sequences_device(v._h, dev, dev, 2, C.byref(sp), C.byref(W.Packed(None, 256, 256, 256, 256)), 8,
                                                          C.byref(n)), b"output buffer is NULL"),
                      (lambda: L.wp_pack_sequences_device(v._h, C.c_void_p(258), dev, 2, C.byref(sp), C.byref(bufs), 8, C.byref(n)), b"4-byte aligned"),
                      (lambda: L.wp_pack_sequences_device(v._h, dev, dev, 2, C.byref(sp), C.byref(W.Packed(256, 256, 257, 256, 256)), 8,
                                                          C.byref(n)), b"4-byte aligned"),
                      (lambda: L.wp_pack_sequences_device(v._h, dev, C.c_void_p(260), 2, C.byref(sp), C.byref(bufs), 8, C.byref(n)), b"8-byte aligned")):
        rc = call()
        assert rc == ARG and msg in L.wp_last_error(), (msg, rc, L.wp_last_error())
    # an unwanted output may be NULL in the device call: the rules pass, and without a GPU the call fails there
    if L.wp_device_count() == 0:
        rc = L.wp_pack_sequences_device(v._h, dev, dev, 2, C.byref(_spec(want=3)), C.byref(W.Packed(256, 256, 256, None, 256)), 8, C.byref(n))
        assert rc == 4 and b"no HIP device" in L.wp_last_error()
    # bad row_splits
    for bad in ([1, 2, 3], [0, 2, 1], [0, -1, 3], [-1, 2, 3]):
        rc, out, rows = _host(v, ids, bad, sp)
        assert rc == ARG and b"row_splits must" in L.wp_last_error() and not any(_blocks(out)), bad
    # sizes: the rows are never dereferenced behind what the rule needs
    rc = L.wp_pack_sequences(v._h, None, None, 2 ** 31, C.byref(sp), C.byref(W.Packed()), C.byref(n))
    assert rc == TOO_LARGE and b"documents" in L.wp_last_error()
    rc = L.wp_pack_sequences_device(v._h, dev, dev, 2 ** 31, C.byref(sp), C.byref(bufs), 8, C.byref(n))
    assert rc == TOO_LARGE and b"documents" in L.wp_last_error()
    one = np.array([1], dtype=np.int32)  # (ids is not read before the totals are checked)
    rc, out, rows = _host(v, one, [0, 2 ** 31], sp)
    assert rc == TOO_LARGE and b"more ids" in L.wp_last_error() and not any(_blocks(out))
    # n_ids fits, N does not: I32_MAX ids in documents of one id need a special each ... stated with few documents:
    # split mode, B = 1: every id is a unit of two cells
    rc, out, rows = _host(v, one, [0, 2 ** 30 + 5], _spec(max_len=2, eos_id=9, long_docs=1))
    assert rc == TOO_LARGE and b"more cells" in L.wp_last_error() and not any(_blocks(out))
    # stream mode: N fits, and the last row rounds n_out * max_len up past INT32_MAX
    rc, out, rows = _host(v, one, [0, I32_MAX - 2], _spec(max_len=2 ** 30 + 7, mode=1))
    assert rc == TOO_LARGE and b"n_out * max_len" in L.wp_last_error() and not any(_blocks(out))
    # the Python mirror's own rules
    with pytest.raises(W.WordPieceError, match="mode must be"):
        v.pack_sequences(ids, splits, mode="best_fit")
    with pytest.raises(W.WordPieceError, match="long_docs must be"):
        v.pack_sequences(ids, splits, long_docs="drop")
    with pytest.raises(W.WordPieceError, match="want names"):
        v.pack_sequences(ids, splits, want=("attention_mask",))
    with pytest.raises(W.WordPieceError, match="end behind the ids"):
        v.pack_sequences(ids, [0, 2, 4])


def test_batches_without_rows_need_no_device():
    L = W.lib()
    v = W.Vocab(VOCAB)
    for splits, n_docs in (([0], 0), ([0, 0], 1), ([0, 0, 0, 0], 3)):
        for mode in ("next_fit", "stream"):
            for long_docs in ("truncate", "split"):
                out = v.pack_sequences([], splits, max_len=5, mode=mode, eos_id=2, long_docs=long_docs, want=("source",))
                assert sorted(out) == ["input_ids", "lengths", "source"]
                assert out["input_ids"].shape == out["source"].shape == (0, 5) and out["lengths"].shape == (0,)
                exp = M.pack([], splits, 5, M.MODES[mode], -1, 2, 0, M.LONG_DOCS[long_docs])["stats"]
                assert v.pack_stats() == exp == dict(n_docs=n_docs, n_empty=n_docs, n_cut=0, n_ids_cut=0, n_pieces=0, n_out=0, n_cells=0,
                                                     n_segments=0)
    # through the C ABI: NULL blocks, n_out 0; ids may be NULL where there are none
    rc, out, rows = _host(v, None, [0, 0], _spec())
    assert rc == 0 and rows == 0 and not any(_blocks(out))
    n = C.c_size_t(5)
    assert L.wp_pack_sequences_device(v._h, None, C.c_void_p(256), 0, C.byref(_spec()), C.byref(W.Packed()), 0, C.byref(n)) == 0
    assert n.value == 0 and v.pack_stats()["n_docs"] == 0


def test_no_cpu_fallback_for_packing():
    if W.lib().wp_device_count() > 0:
        pytest.skip("GPU present")
    v = W.Vocab(VOCAB)
    with pytest.raises(W.WordPieceError, match="no HIP device"):
        v.pack_sequences([1, 2, 1], [0, 2, 3], max_len=4)
    n = C.c_size_t()
    dev = C.c_void_p(256)
    rc = W.lib().wp_pack_sequences_device(v._h, dev, dev, 1, C.byref(_spec()), C.byref(W.Packed(256, 256, 256, 256, 256)), 4, C.byref(n))
    assert rc == 4 and b"no HIP device" in W.lib().wp_last_error()  # WP_ERR_NO_DEVICE
