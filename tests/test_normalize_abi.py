"""CPU checks of WP_OPT_NORMALIZE at the C ABI: argument errors, what needs no device, the layout of wp_stats and wp_norm_stats."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import wordpiece_amd as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = ["[UNK]", "hello", "cafe", "##s", "world"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(W.LIB_PATH):
        from wordpiece_amd import build
        build.build()


def test_symbols_and_constants():
    L = W.lib()
    for s in ("wp_normalize_cp", "wp_normalize_device", "wp_normalize", "wp_get_norm_stats"):
        assert s in W.ABI_SYMBOLS and hasattr(L, s)
    assert (W.WP_OPT_NORMALIZE, W.WP_NORM_CLEAN, W.WP_NORM_LOWER, W.WP_NORM_STRIP_ACCENTS, W.WP_NORM_BERT_UNCASED) == (14, 1, 2, 4, 7)


def test_unknown_flag_bits_are_an_argument_error():
    v = W.Vocab(VOCAB)
    L = W.lib()
    for bad in (8, 15, 16, 1 << 20, -1):
        assert L.wp_set_option(v._h, W.WP_OPT_NORMALIZE, bad) == 6 and b"NORMALIZE" in L.wp_last_error()  # WP_ERR_ARG
        with pytest.raises(W.WordPieceError, match="flag"):
            W.Vocab(VOCAB, normalize=bad)
        out, n = C.c_void_p(), C.c_size_t()
        assert L.wp_normalize(v._h, b"a", 1, bad, C.byref(out), C.byref(n)) == 6
        assert L.wp_normalize_device(v._h, None, 0, bad, C.byref(out), C.byref(n)) == 6
    for ok in range(8):
        v.set_option(W.WP_OPT_NORMALIZE, ok)


def test_empty_text_needs_no_device():
    v = W.Vocab(VOCAB, normalize=W.WP_NORM_BERT_UNCASED)
    assert len(v.encode(b"")) == 0 and len(v.fast_encode(b"")) == 0
    ids, offs = v.encode_with_offsets(b"", unit="char")
    assert len(ids) == 0 and offs.shape == (0, 2)
    ids, splits = v.encode_rows(docs=["", ""])
    assert len(ids) == 0 and splits.tolist() == [0, 0, 0]
    assert v.normalize(b"") == b"" and v.normalize("", flags=1) == b""
    assert v.stats()["normalize"] == 0  # (no encode ran)


def test_no_cpu_fallback():
    if W.lib().wp_device_count() > 0:
        pytest.skip("GPU present")
    v = W.Vocab(VOCAB, normalize=7)
    L = W.lib()
    ids, n = C.POINTER(C.c_int32)(), C.c_size_t()
    assert L.wp_linear_encode(v._h, b"Hello", 5, C.byref(ids), C.byref(n)) == 4  # WP_ERR_NO_DEVICE
    for call in (lambda: v.encode("Hello"), lambda: v.fast_encode("Hello"), lambda: v.encode_with_offsets("Hello"),
                 lambda: v.encode_rows(docs=["Hello"]), lambda: v.normalize("Hello"), lambda: v.normalize("Hello", flags=0)):
        with pytest.raises(W.WordPieceError, match="no HIP device"):
            call()


def test_stats_mirrors_match_the_c_structs(tmp_path):
    """wp_stats keeps its layout (the new statistics have a struct of their own); both mirrors have the C sizes"""
    assert [f[0] for f in W.NormStats._fields_] == ["normalize", "norm_bytes", "ms_normalize"]
    assert [f[0] for f in W.Stats._fields_][-1] == "rows_route"
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(wp_stats), offsetof(wp_stats, rows_route), '
                   'sizeof(wp_norm_stats), offsetof(wp_norm_stats, ms_normalize)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(W.Stats), W.Stats.rows_route.offset, C.sizeof(W.NormStats), W.NormStats.ms_normalize.offset]
    assert np.dtype(np.int64).itemsize == 8
