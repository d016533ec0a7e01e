"""CPU checks of best-fit packing: header and exported symbols against the ctypes mirrors, every argument rule before a
device, and the planner (wp_binpack_plan) against the literal procedure of tests/binpack_model.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import binpack_model as M
import wordpiece_amd as W
from wordpiece_amd import binpack as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = 6


def test_symbols_and_structs_match_the_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd_binpack.h")).read()
    assert sorted(re.findall(r"\b(wp_\w+)\s*\(", hdr.split("#ifndef")[1])) == sorted(B.ABI_SYMBOLS)
    assert all(hasattr(B.lib(), name) and name not in W.ABI_SYMBOLS for name in B.ABI_SYMBOLS)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd_binpack.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(wp_binpack_spec), offsetof(wp_binpack_spec, reserved1),\n'
                   '         sizeof(wp_binpack_run), offsetof(wp_binpack_run, col0), sizeof(wp_binpack_row_range), offsetof(wp_binpack_row_range, cells_per_row),\n'
                   '         sizeof(wp_binpack_plan_result), offsetof(wp_binpack_plan_result, row_ranges), sizeof(wp_binpack_stats),\n'
                   '         offsetof(wp_binpack_stats, n_row_ranges), WP_BINPACK_MAX_LEN);\n  return 0;\n}\n')
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "sz"), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "sz")], check=True, capture_output=True, text=True).stdout.split()]
    S, R, G, P, T = B.BinpackSpec, B.BinpackRun, B.BinpackRowRange, B.BinpackPlan, B.BinpackStats
    assert got == [C.sizeof(S), S.reserved1.offset, C.sizeof(R), R.col0.offset, C.sizeof(G), G.cells_per_row.offset, C.sizeof(P), P.row_ranges.offset,
                   C.sizeof(T), T.n_row_ranges.offset, B.WP_BINPACK_MAX_LEN]
    assert (C.sizeof(S), C.sizeof(R), C.sizeof(G), C.sizeof(P), C.sizeof(T)) == (32, 40, 40, 56, 80)


def _call(v, spec, device, ids=(5, 6, 7), splits=(0, 2, 3), out=True, n_out=True, d_ptr=256):
    """-> (rc, Packed, n): the host form on arrays, or the device form on pointers that are never dereferenced"""
    o, n = W.Packed(*range(1, 6)), C.c_size_t(77)
    sp, op, np_ = None if spec is None else C.byref(spec), C.byref(o) if out else None, C.byref(n) if n_out else None
    n_docs = 2 if splits is None else len(splits) - 1
    if device:
        rc = B.lib().wp_pack_best_fit_device(v._h, C.c_void_p(d_ptr), None if splits is None else C.c_void_p(512), n_docs, sp, op, 4, np_)
    else:
        a, s = None if ids is None else np.asarray(ids, np.int32), None if splits is None else np.asarray(splits, np.int64)
        rc = B.lib().wp_pack_best_fit(v._h, W._i32_ptr(a), W._i64_ptr(s), n_docs, sp, op, np_)
    return rc, o, n.value


BAD_SPECS = [(dict(long_docs=2), b"unknown long_docs"), (dict(want=8), b"want has bits outside 7"), (dict(max_len=0), b"max_len must be at least 1"),
             (dict(max_len=8193), b"max_len must be at most 8192"), (dict(max_len=2, bos_id=1, eos_id=2), b"max_len leaves no room"),
             (dict(reserved0=1), b"reserved0 must be 0"), (dict(reserved1=-1), b"reserved1 must be 0")]


@pytest.mark.parametrize("fields,msg", BAD_SPECS, ids=[m.decode() for _, m in BAD_SPECS])
def test_argument_errors_come_before_the_device_and_name_the_field(fields, msg):
    v, spec = W.Vocab(["[UNK]", "a"]), B.BinpackSpec(8, -1, -1, 0, 1, 7, 0, 0)
    for name, x in fields.items():
        setattr(spec, name, x)
    for device in (False, True):
        rc, o, n = _call(v, spec, device)
        err = B.lib().wp_last_error()
        assert rc == ARG and msg in err and err.startswith(b"binpack: ") and n == 0, (device, err)
    assert B.binpack_stats(v)["n_docs"] == -1 and v.pack_stats()["n_docs"] == -1  # none of these was a call


def test_pointer_rules_and_calls_without_units():
    v, spec, last = W.Vocab(["[UNK]", "a"]), B.BinpackSpec(8, -1, -1, 0, 1, 7, 0, 0), B.lib().wp_last_error
    for device in (False, True):
        assert _call(v, None, device)[0] == ARG and b"binpack: spec is NULL" in last()
        assert _call(v, spec, device, n_out=False)[0] == ARG and b"binpack: an out-pointer is NULL" in last()
        assert _call(v, spec, device, out=False)[0] == ARG and b"binpack: an out-pointer is NULL" in last()
        assert _call(v, spec, device, splits=None)[0] == ARG and b"binpack: row_splits is NULL" in last()
    assert _call(v, spec, True, d_ptr=258)[0] == ARG and b"binpack: device ids and outputs must be 4-byte aligned" in last()
    assert _call(v, spec, False, ids=None)[0] == ARG and b"binpack: ids is NULL" in last()
    assert _call(v, spec, False, splits=(1, 2, 3))[0] == ARG and b"binpack: row_splits must start at 0" in last()
    assert _call(v, spec, False, splits=(0, 3, 2))[0] == ARG and b"binpack: row_splits must never descend" in last()
    assert B.binpack_stats(v)["n_docs"] == -1
    with pytest.raises(W.WordPieceError, match="long_docs must be"):
        B.pack_best_fit(v, [1], [0, 1], long_docs="best")
    for splits in ([0], [0, 0, 0, 0]):  # no document, empty documents only: answered without a device
        got = B.pack_best_fit(v, [], splits, max_len=8)
        assert got["input_ids"].shape == (0, 8) and got["lengths"].shape == (0,)
        assert B.binpack_stats(v) == dict(n_docs=len(splits) - 1, n_empty=len(splits) - 1, n_cut=0, n_ids_cut=0, n_pieces=0, n_out=0, n_cells=0,
                                          n_segments=0, n_runs=0, n_row_ranges=0)
    assert v.pack_stats()["n_docs"] == -1


def _random_hist(seed):
    rng, L = np.random.default_rng(seed), (5, 128, 512)[seed % 3]
    return L, {int(u): int(c) for u, c in zip(rng.integers(1, L + 1, L // 2 + 2), rng.integers(1, 40, L // 2 + 2))}


HISTS = [("single unit", 7, {3: 1}), ("all units L", 5, {5: 9}), ("all units 1, L 8192", 8192, {1: 20000}), ("L 1", 1, {1: 4}),
         ("one partly filled row", 10, {4: 5}), ("a group splits three ways", 10, {6: 5, 2: 5, 1: 3})] + \
        [("random %d" % s,) + _random_hist(s) for s in range(10)]


@pytest.mark.parametrize("L,hist", [h[1:] for h in HISTS], ids=[h[0] for h in HISTS])
def test_plan_against_the_model(L, hist):
    h = np.zeros(L + 1, np.int64)
    for u, c in hist.items():
        h[u] = c
    u = np.random.default_rng(L).permutation(np.repeat(np.arange(L + 1), h))  # the units in some document order
    row, slot, col, n_out = M.place(u, L)
    plan = B.plan_best_fit(h, L)
    assert (plan["n_out"], plan["n_units"], plan["n_cells"]) == (n_out, len(u), int(u.sum()))
    assert plan["n_out"] == B.plan_best_fit(u, L, lengths=True)["n_out"]
    sigma = np.argsort(-u, kind="stable")
    got = M.expand(plan["runs"], len(u))  # (asserts that the runs tile the ranks)
    for name, exp, have in (("row", row, got[0]), ("slot", slot, got[1]), ("col", col, got[2]), ("unit", u, got[3])):
        assert np.array_equal(exp[sigma], have), name
    g = plan["row_ranges"]
    units, cells = np.bincount(row, minlength=n_out), np.bincount(row, weights=u, minlength=n_out).astype(np.int64)
    assert g["row0"].tolist() == (np.cumsum(g["n_rows"]) - g["n_rows"]).tolist() and g["n_rows"].sum() == n_out and np.all(g["n_rows"] >= 1)
    assert np.array_equal(np.repeat(g["units_per_row"], g["n_rows"]), units) and np.array_equal(np.repeat(g["cells_per_row"], g["n_rows"]), cells)
    assert np.array_equal(g["first_unit"], (np.cumsum(units) - units)[g["row0"]]) and np.array_equal(g["first_cell"], (np.cumsum(cells) - cells)[g["row0"]])
    assert not np.any((g["units_per_row"][1:] == g["units_per_row"][:-1]) & (g["cells_per_row"][1:] == g["cells_per_row"][:-1]))  # maximal
