"""CPU tests of wp_refine_sched (include/wordpiece_amd.h): where the refinement of the last encode was queued, in a struct of
its own beside wp_refine_stats.  The ctypes mirror follows the header, both have the size and offsets a C compiler gives the
header's struct, a handle that never encoded reports zeros, and NULL arguments are argument errors."""
import ctypes as C
import os
import re
import subprocess

import wordpiece_amd as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WP_ERR_ARG = 6


def _header():
    with open(os.path.join(ROOT, "include", "wordpiece_amd.h")) as f:
        return f.read()


def test_refine_sched_struct_matches_header(tmp_path):
    hdr = _header()
    end = hdr.index("} wp_refine_sched;")
    body = hdr[hdr.rindex("typedef struct {", 0, end):end]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("typedef struct {", "")
    fields = [tuple(decl.split()) for decl in body.split(";") if decl.strip()]
    widths = {"int32_t": C.c_int32, "double": C.c_double}
    assert [(name, widths[ctype]) for ctype, name in fields] == list(W.RefineSched._fields_)
    assert [name for _, name in fields] == ["early", "reserved", "ms_sort_to_scan"]
    # wp_stats and wp_refine_stats keep their sizes
    probe = ["sizeof(wp_refine_sched)"] + ["offsetof(wp_refine_sched, %s)" % name for _, name in fields] + \
            ["sizeof(wp_stats)", "sizeof(wp_refine_stats)"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd.h"\nint main(void) {\n' +
                   "".join('  printf("%%zu ", (size_t)%s);\n' % p for p in probe) + "  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(W.RefineSched)] + [getattr(W.RefineSched, name).offset for _, name in fields] + \
                  [C.sizeof(W.Stats), C.sizeof(W.RefineStats)]
    assert C.sizeof(W.RefineSched) == 16 and C.sizeof(W.RefineStats) == 56


def test_option_number_is_the_headers():
    m = re.search(r"#define WP_OPT_LATE_REFINE (\d+)", _header())
    assert m and int(m.group(1)) == W.WP_OPT_LATE_REFINE == 15
    numbers = [int(v) for v in re.findall(r"#define WP_OPT_\w+ (\d+)", _header())]
    assert len(set(numbers)) == len(numbers) and max(numbers) == W.WP_OPT_LATE_REFINE
    gv = W.Vocab(["a"])
    gv.set_option(W.WP_OPT_LATE_REFINE, 1)  # (accepted without a device)
    gv.set_option(W.WP_OPT_LATE_REFINE, 0)


def test_zero_before_any_encode():
    gv = W.Vocab(["a"])
    assert gv.refine_sched() == dict(early=0, ms_sort_to_scan=0.0)
    assert gv.encode("") .tolist() == [] and gv.refine_sched() == dict(early=0, ms_sort_to_scan=0.0)


def test_null_arguments_are_argument_errors():
    L = W.lib()
    gv = W.Vocab(["a"])
    out = W.RefineSched()
    assert L.wp_get_refine_sched(None, C.byref(out)) == WP_ERR_ARG
    assert b"wp_get_refine_sched" in L.wp_last_error()
    assert L.wp_get_refine_sched(gv._h, None) == WP_ERR_ARG
    assert L.wp_get_refine_sched(gv._h, C.byref(out)) == 0
