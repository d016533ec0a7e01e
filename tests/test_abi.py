"""CPU checks of the host side: the C-ABI library loads and exports every symbol the header
declares, the host vocab logic matches the oracle, and compute entry points fail loudly
without a GPU (no fallback)."""
import os
import re

import pytest

import oracle_lib as O
import wordpiece_amd as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built():
    if not os.path.exists(W.LIB_PATH):
        from wordpiece_amd import build
        build.build()


def test_header_symbols_exported():
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd.h")).read()
    declared = set(re.findall(r"\b(wp_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(W.ABI_SYMBOLS)
    L = W.lib()
    for s in declared:
        assert hasattr(L, s), s


def test_vocab_classification_matches_oracle():
    words = ["a", "##a", "[UNK]", "[a]", "##[a]", "...", ".", "##..", "a.", "[]", "#", "###", "####", "[ ]", ", ",
             "aé中", "##中", "a b", "[CLS", "CLS]", b"\xffa", b"##\xffb"]
    gv, ov = W.Vocab(words), O.Vocab(words)
    assert len(gv) == ov.size and gv.unk_id == ov.unk_id == 2
    for i in range(len(words)):
        assert gv.token_flags(i) == ov.flags(i), words[i]
        assert gv.token_len(i) == len(ov.word(i)), words[i]


def test_empty_word_error_message():
    for bad in (["a", "##"], ["a", ""], [b"\xff"]):
        with pytest.raises(W.WordPieceError, match="Vocab word is empty"):
            W.Vocab(bad)


def test_vocab_from_file_getline_semantics(tmp_path):
    p = tmp_path / "vocab.txt"
    p.write_bytes(b"[UNK]\na\r\n##b\nlast")
    v = W.Vocab(file=str(p))
    assert len(v) == 4 and v.unk_id == 0
    assert v.token_len(1) == 2  # the CR stays in the token (utils.cpp:123-137)


def test_empty_text_needs_no_device():
    assert W.linear.encode("", ["a"]) == []


def test_no_cpu_fallback():
    if W.lib().wp_device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(W.WordPieceError, match="no HIP device"):
        W.linear.encode("ab", ["a", "##b"])


def test_shard_bounds_cut_at_whitespace():
    data = b"alpha beta\tgamma\ndelta epsilon zeta"
    for ws in (1, 2, 3, 4, 8):
        b = W.shard_bounds(data, ws)
        assert b[0][0] == 0 and b[-1][1] == len(data)
        for (s0, e0), (s1, e1) in zip(b, b[1:]):
            assert e0 == s1
            assert e0 == len(data) or data[e0] in b" \t\n"


def test_file_entry_points_report_missing_files(tmp_path):
    """linear.cpp:337-374: a missing text file throws (Boost's mapped_file there, mmap here); a missing
    vocab file is an empty vocabulary (std::ifstream reads nothing, utils.cpp:123-137) and an output
    file that cannot be created is an error.  All before the device is needed."""
    vf = tmp_path / "v.txt"
    vf.write_text("a\nb\n")
    with pytest.raises(W.WordPieceError, match="cannot open"):
        W.linear.encode(str(tmp_path / "missing.txt"), str(vf))
    with pytest.raises(W.WordPieceError, match="cannot open"):
        W.linear.encodeExternal(str(vf), str(vf), str(tmp_path / "no_such_dir" / "out.txt"), 1000)
    with pytest.raises(W.WordPieceError, match="memory_limit too small"):
        W.linear.encodeExternal(str(vf), str(vf), str(tmp_path / "out.txt"), 10)
    empty = tmp_path / "empty.txt"
    empty.write_bytes(b"")
    assert W.linear.encode(str(empty), str(tmp_path / "missing_vocab.txt")) == []  # nothing to encode, nothing loaded


def test_stats_struct_matches_header():
    """The ctypes mirror of wp_stats (field order, widths, the array) follows include/wordpiece_amd.h, and the
    option numbers of the Python module are the header's."""
    import ctypes as C
    import re
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd.h")).read()
    body = hdr[hdr.index("typedef struct {", hdr.index("statistics of the last encode")):hdr.index("} wp_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.replace("typedef struct {", "").strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for name in names.split(","):
            name = name.strip()
            m = re.match(r"(\w+)\[(\d+)\]", name)
            fields.append((m.group(1), ctype, int(m.group(2))) if m else (name, ctype, 0))
    widths = {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}
    mirror = W.Stats._fields_
    assert [f[0] for f in fields] == [f[0] for f in mirror]
    for (name, ctype, count), (_, pytype) in zip(fields, mirror):
        want = widths[ctype] * count if count else widths[ctype]
        assert C.sizeof(pytype) == C.sizeof(want), name
    for name, value in re.findall(r"#define (WP_OPT_\w+) (\d+)", hdr):
        assert getattr(W, name) == int(value), name


def test_walk_stats_struct_matches_header(tmp_path):
    """wp_walk_stats is a struct of its own (wp_stats keeps its size and its last field): the ctypes mirror follows the
    header's fields, and both mirrors have the sizes and offsets a C compiler gives the header's structs."""
    import ctypes as C
    import subprocess
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd.h")).read()
    body = hdr[hdr.rindex("typedef struct {", 0, hdr.index("} wp_walk_stats;")):hdr.index("} wp_walk_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("typedef struct {", "")
    fields = [tuple(decl.split()) for decl in body.split(";") if decl.strip()]
    widths = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    assert [(name, widths[ctype]) for ctype, name in fields] == list(W.WalkStats._fields_)
    assert [name for _, name in fields] == ["n_wide_words", "n_long_words", "lean", "max_anchor_gap"]
    assert [f[0] for f in W.Stats._fields_][-1] == "rows_route"
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(wp_stats), offsetof(wp_stats, rows_route), '
                   'sizeof(wp_walk_stats), offsetof(wp_walk_stats, lean), offsetof(wp_walk_stats, max_anchor_gap)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(W.Stats), W.Stats.rows_route.offset, C.sizeof(W.WalkStats), W.WalkStats.lean.offset,
                   W.WalkStats.max_anchor_gap.offset]
    # without a device the statistics of a handle that never encoded are zero
    ws = W.Vocab(["a"]).walk_stats()
    assert ws == dict(n_wide_words=0, n_long_words=0, lean=0, max_anchor_gap=0)


def test_refine_stats_struct_matches_header(tmp_path):
    """wp_refine_stats is a struct of its own (wp_stats keeps its size and its last field): the ctypes mirror follows the
    header's fields, and both mirrors have the sizes and offsets a C compiler gives the header's structs."""
    import ctypes as C
    import subprocess
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd.h")).read()
    body = hdr[hdr.rindex("typedef struct {", 0, hdr.index("} wp_refine_stats;")):hdr.index("} wp_refine_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("typedef struct {", "")
    fields = [tuple(decl.split()) for decl in body.split(";") if decl.strip()]
    widths = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    assert [(name, widths[ctype]) for ctype, name in fields] == list(W.RefineStats._fields_)
    assert [name for _, name in fields] == ["n_groups", "n_entries", "n_large_groups", "n_large_entries", "trie_nodes",
                                            "sort_bits", "key_lookup", "symbol_bytes", "reserved"]
    assert [f[0] for f in W.Stats._fields_][-1] == "rows_route"
    probe = ["sizeof(wp_stats)", "offsetof(wp_stats, rows_route)", "sizeof(wp_walk_stats)", "sizeof(wp_refine_stats)"] + \
            ["offsetof(wp_refine_stats, %s)" % name for _, name in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd.h"\nint main(void) {\n' +
                   "".join('  printf("%%zu ", (size_t)%s);\n' % p for p in probe) + "  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(W.Stats), W.Stats.rows_route.offset, C.sizeof(W.WalkStats), C.sizeof(W.RefineStats)] + \
                  [getattr(W.RefineStats, name).offset for _, name in fields]
    assert C.sizeof(W.RefineStats) == 56
    # without a device the statistics of a handle that never encoded are zero
    rs = W.Vocab(["a"]).refine_stats()
    assert rs == dict(n_groups=0, n_entries=0, n_large_groups=0, n_large_entries=0, trie_nodes=0, sort_bits=0, key_lookup=0,
                      symbol_bytes=0)


def test_step_stats_struct_matches_header(tmp_path):
    """wp_step_stats is a struct of its own (the other statistics structs keep their sizes): the ctypes mirror follows the
    header's fields, and has the size and offsets a C compiler gives the header's struct; NULL arguments are argument errors."""
    import ctypes as C
    import subprocess
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd.h")).read()
    end = hdr.index("} wp_step_stats;")
    body = hdr[hdr.rindex("typedef struct {", 0, end):end]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("typedef struct {", "")
    fields = [tuple(decl.split()) for decl in body.split(";") if decl.strip()]
    widths = {"int64_t": C.c_int64, "int32_t": C.c_int32}
    assert [(name, widths[ctype]) for ctype, name in fields] == list(W.StepStats._fields_)
    assert [name for _, name in fields] == ["n_marks", "n_steps", "n_tiles", "n_groups_of_tiles", "bucket_shift", "bucket_shift_all",
                                            "key_shift", "key_shift_all", "packed", "key_lookup"]
    probe = ["sizeof(wp_step_stats)"] + ["offsetof(wp_step_stats, %s)" % name for _, name in fields] + \
            ["sizeof(wp_stats)", "sizeof(wp_walk_stats)", "sizeof(wp_refine_stats)", "sizeof(wp_refine_sched)"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd.h"\nint main(void) {\n' +
                   "".join('  printf("%%zu ", (size_t)%s);\n' % p for p in probe) + "  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(W.StepStats)] + [getattr(W.StepStats, name).offset for _, name in fields] + \
                  [C.sizeof(W.Stats), C.sizeof(W.WalkStats), C.sizeof(W.RefineStats), C.sizeof(W.RefineSched)]
    assert C.sizeof(W.StepStats) == 56 and C.sizeof(W.RefineStats) == 56 and C.sizeof(W.RefineSched) == 16
    # without a device the statistics of a handle that never encoded are zero; WP_OPT_KEEP_DEBUG takes 0, 1 and 2
    gv = W.Vocab(["a"])
    assert gv.step_stats() == {name: 0 for _, name in fields}
    for value in (2, 1, 0):
        gv.set_option(W.WP_OPT_KEEP_DEBUG, value)
    L = W.lib()
    out = W.StepStats()
    assert L.wp_get_step_stats(None, C.byref(out)) == 6 and b"wp_get_step_stats" in L.wp_last_error()
    assert L.wp_get_step_stats(gv._h, None) == 6 and L.wp_get_step_stats(gv._h, C.byref(out)) == 0
