"""The tables of WP_OPT_NORMALIZE (csrc/normalize_tables.h) without a GPU: wp_normalize_cp reads what the kernels read."""
import ctypes as C
import os
import re
import subprocess
import sys
import unicodedata

import pytest

import normalize_model as NM
import wordpiece_amd as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "wordpiece_amd", "csrc", "normalize_tables.h")


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(W.LIB_PATH):
        from wordpiece_amd import build
        build.build()


def _header_version():
    with open(HEADER) as f:
        return re.search(r'#define WP_NORM_UNICODE_VERSION "([0-9.]+)"', f.read()).group(1)


def _same_unicode():
    have, want = unicodedata.unidata_version, _header_version()
    if have != want:
        pytest.skip("this Python's unicodedata is Unicode %s, the committed tables are Unicode %s" % (have, want))


def test_every_code_point_and_flag_set_against_the_model():
    _same_unicode()
    fn = W.lib().wp_normalize_cp
    out = (C.c_uint32 * 3)()
    for flags in NM.FLAG_SETS:
        bad = []
        for cp in range(0x110000):
            n = fn(flags, cp, out)
            if 0xD800 <= cp < 0xE000:
                assert n == -1
                continue
            if out[:n] != NM.normalize_cp(flags, cp):
                bad.append(cp)
        assert not bad, "flags %d: %d code points differ, first U+%04X" % (flags, len(bad), bad[0])


def test_generator_reproduces_the_committed_header(tmp_path):
    _same_unicode()
    out = tmp_path / "normalize_tables.h"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_normalize_tables.py"), str(out)], check=True)
    with open(HEADER, "rb") as f:
        assert out.read_bytes() == f.read()


def test_values_outside_the_rule():
    out = (C.c_uint32 * 3)()
    fn = W.lib().wp_normalize_cp
    assert fn(7, 0x110000, out) == -1 and fn(7, 0xFFFFFFFF, out) == -1 and fn(7, 0xDFFF, out) == -1
    assert fn(8, 0x41, out) == -1 and fn(-1, 0x41, out) == -1
    assert W.normalize_cp(0, 0x41) == [0x41] and W.normalize_cp(0, 0) == [0]  # no flags: every code point is itself
    assert W.normalize_cp(7, 0xD800) is None and W.normalize_cp(16, 0x41) is None


def test_pinned_code_points():
    assert W.normalize_cp(2, ord("A")) == [ord("a")] and W.normalize_cp(5, ord("A")) == [ord("A")]
    assert W.normalize_cp(2, 0x130) == [0x69, 0x307] and W.normalize_cp(6, 0x130) == [0x69]
    assert W.normalize_cp(4, 0xE9) == [0x65] and W.normalize_cp(2, 0xC9) == [0xE9] and W.normalize_cp(6, 0xC9) == [0x65]
    assert W.normalize_cp(4, 0xAC00) == [0x1100, 0x1161] and W.normalize_cp(7, 0xAC01) == [0x1100, 0x1161, 0x11A8]
    assert W.normalize_cp(2, 0xAC01) == [0xAC01]
    assert W.normalize_cp(1, 0xA0) == [0x20] and W.normalize_cp(6, 0xA0) == [0xA0] and W.normalize_cp(1, 0x3000) == [0x20]
    for cp in (0x00, 0x01, 0x0B, 0x0C, 0x1F, 0x7F, 0x85, 0xAD, 0x200B, 0x200D, 0xFEFF, 0xFFFD, 0xE0001):
        assert W.normalize_cp(1, cp) == [] and W.normalize_cp(6, cp) != []
    for cp in (0x09, 0x0A, 0x0D, 0x20):
        assert W.normalize_cp(7, cp) == [cp]
    assert W.normalize_cp(4, 0x301) == [] and W.normalize_cp(3, 0x301) == [0x301]
    assert W.normalize_cp(2, 0x3A3) == [0x3C3]  # no final sigma: the rule sees one code point
