"""The class table of the quality signals (csrc/class_tables.h, tools/gen_class_tables.py): the generator reproduces the
committed header, and the table the library reads holds unicodedata's categories for every code point."""
import os
import re
import subprocess
import sys
import unicodedata

import pytest

import wordpiece_amd as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "wordpiece_amd", "csrc", "class_tables.h")


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(W.LIB_PATH):
        from wordpiece_amd import build
        build.build()


def _same_unicode():
    with open(HEADER) as f:
        version = re.search(r'#define WP_CLASS_UNICODE_VERSION "([0-9.]+)"', f.read()).group(1)
    if version != unicodedata.unidata_version:
        pytest.skip("the header was generated from Unicode %s, this Python has %s" % (version, unicodedata.unidata_version))


def test_generator_reproduces_the_committed_header(tmp_path):
    _same_unicode()
    out = tmp_path / "class_tables.h"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_class_tables.py"), str(out)], check=True)
    with open(HEADER, "rb") as f:
        assert out.read_bytes() == f.read()


def test_every_code_point_has_unicodedatas_class():
    _same_unicode()
    fn = W.lib().wp_quality_class
    bad = []
    for cp in range(0x110000):
        if 0xD800 <= cp < 0xE000:
            continue
        cat = unicodedata.category(chr(cp))
        exp = (1 if cat[0] == "L" else 0) | (2 if cat == "Nd" else 0) | (4 if cat == "Lu" else 0)
        if fn(cp) != exp:
            bad.append(cp)
    assert not bad, "%d code points differ, first U+%04X" % (len(bad), bad[0])


def test_values_outside_the_code_points():
    fn = W.lib().wp_quality_class
    assert fn(0x110000) == -1 and fn(0xFFFFFFFF) == -1 and fn(0xD800) == -1 and fn(0xDFFF) == -1
    assert fn(ord("A")) == 5 and fn(ord("a")) == 1 and fn(ord("7")) == 2 and fn(ord(" ")) == 0 and fn(0x4E2D) == 1
