"""GPU tests (-m gpu) of the documents layer — csrc/rows.h, the three kernels a normalised handle adds in csrc/normalize.h and
LinearPath::row_structure — on the inputs of rows_cases.py.  For every named case of families L (line ends), S (starts to
ids), B (the rebase), N (a normalised handle, flag sets 1, 4 and 7) and C (composed, three line tiles):

  - wp_linear_encode_rows with the explicit starts of the rows, with the lines of the text, and with the lines of the text
    without its last byte (the open end), wherever the case's text ends in '\n'; a text that is open-ended as built runs as
    it stands;
  - in every unit (none, bytes, code points): ids, row_splits and offsets equal the model's, exactly (rows_cases.expected: row
    i is the encode of document i alone; a normalised handle: normalize_model per document);
  - wp_stats: n_rows, rows_route == 1, offsets_unit, n_ids, normalize.

Family P (test_pack_edge, one test per max_len of rows_cases.MAX_LENS, every lane-group width): wp_linear_encode_padded over
the combinations of cls_id / sep_id that fit, 1, r - 1, r, r + 1 and 3 r + 2 rows (r: the rows of a workgroup) and row
lengths 0, keep - 1, keep, keep + 1 and 3 max_len: cells and lengths against rows_model.pack, rows_truncated against its
count, and the device form into caller-owned tensors with three sentinel rows behind n_rows, which stay untouched (explicit
starts and lines in turn).

A subset (rows_cases.SUBSET, SUBSET_MAX_LENS: at least one case per family) runs once more in the bounds-checking build (a child
process) and once with WP_OPT_ARENA_GUARD.  Not repeated here: dirty bytes behind nbytes (test_gpu_decode_edges.py), the
per-document route, capacity errors and the messages of rows_check_kernel (test_gpu_rows.py).

Wall time (measured on an MI355X): 7.5 s for the 142 tests of this file — 3.1 s the bounds-checking child, 0.7 s the arena-guard
subset, no other test above 0.25 s (tests/test_gpu_rows.py takes 219 s in the same job).

Found by this file: no disagreement between the library and the models.  Against eight deliberately wrong scratch builds
(value-only mutations, never committed; the 141 tests without the bounds-checking child, which loads a library of its own):
  (1) the open-end rule of line_ends16 with `<` for `<=`: 11 fail — L_len_16_open, L_len_32_open, L_len_32_open_blank,
      L_len_T_open, L_len_2T_open, L_8a_open_end, and through their open ends (whole chunks without the last byte)
      L_len_17_nl, L_len_T+1_nl, S_behind_5_2 and B_rows_2048; the arena-guard subset (L_len_T_open).
  (2) `| x` dropped from its zero-byte test: 8 fail — the six L_8a_*_chunk / _tile cases, C_plain, the arena-guard subset.
  (3) `lo = q` for `lo = q + 1` in the gallop of cp_at_byte: nothing fails, and nothing can — byte_of[q] < b holds where the
      assignment stands, so the bisection over [q, hi) returns what the one over [q + 1, hi) returns (one load more).  In
      its place the gallop's comparison with `<=` for `<`, which is wrong only where a probe reads the answer's own entry:
      37 fail — all seven S_probe_hit_* (added for it), the nine S_behind_*, S_first_invalid, B_rows_2048 / _2049, ten N
      cases, both C cases, L_invalid_lines and four L_8a cases.
  (4) `<` for `<=` in row_of_id: 100 fail — every case with an id behind the first row (37 L, 22 S, 11 B, 27 N, 2 C);
      the 18 that pass have no id behind their first row.
  (5) `r_hi` for `r_hi + 1` in rebase_kernel: 96 fail (34 L, 22 S, 10 B, 27 N, 2 C); B_empty_300 and L_nl_T-1 / _T / _T-1_T
      pass, as they must: every rebase tile of theirs lies inside one row.
  (6) `col <= head + keep` in the id branch of pack_rows_kernel: all 16 test_pack_edge and the arena-guard subset fail.
  (7) `<=` for `<` in norm_doc_starts_kernel: 29 fail — 27 of the 33 N cases (all but the six N_only_dropped_all_*, which have
      no ids), C_norm_f7, the arena-guard subset.
Of the existing suite (test_gpu_rows.py::test_golden_and_random_batches, ::test_medium_inputs_on_every_path and
test_gpu_normalize.py::test_documents_both_routes, run against the same builds): (1) fails the first, (2) the second and the
third, (4) and (5) all three, (7) the third, (3) none; (6) was not run against them — some of their batches have no ids, and
the mutant would then read through the null ids pointer.
"""
import functools
import json
import os
import traceback

import numpy as np
import pytest

import round0_cases as R0
import rows_cases as K
import rows_model as R
import wordpiece_amd as W

pytestmark = pytest.mark.gpu
PKG = os.path.dirname(os.path.abspath(W.__file__))
UNITS = (None, "byte", "char")
UNIT_CODE = {None: -1, "byte": 0, "char": 1}


@functools.lru_cache(maxsize=None)
def _handle(vocab, flags, guard=False):
    """one handle per vocabulary and flag set for the whole file: the cases follow each other on it"""
    gv = W.Vocab(list(vocab), normalize=flags)
    if guard:
        gv.set_option(W.WP_OPT_ARENA_GUARD, 1)
    return gv


def _first_difference(got, want):
    n = min(len(got), len(want))
    for i in range(n):
        if got[i] != want[i]:
            return "at %d: %r, expected %r" % (i, got[i], want[i])
    return "lengths %d, expected %d" % (len(got), len(want))


def _same(got, exp, label):
    ids, splits = got[0], got[1]
    assert ids.dtype == np.int32 and splits.dtype == np.int64, label
    assert splits.tolist() == exp[1], (label, "row_splits", _first_difference(splits.tolist(), exp[1]))
    assert ids.tolist() == exp[0], (label, "ids", _first_difference(ids.tolist(), exp[0]))
    if exp[2] is not None:
        assert got[2].dtype == np.uint32 and got[2].shape == (len(exp[0]), 2), label
        offs = [tuple(r) for r in got[2].tolist()]
        assert offs == exp[2], (label, "offsets", _first_difference(offs, exp[2]))
    else:
        assert len(got) == 2, label


def check_case(name, guard=False, debug_build=False):
    c = K.build(name)
    gv = _handle(tuple(c.vocab), c.flags, guard)
    calls = 0
    for label, t, starts, rows in c.runs():
        off = None if starts is None else np.array(starts, dtype=np.int64)
        for unit in UNITS:
            exp = K.expected(c, rows, unit)
            got = gv.encode_rows(text=t, doc_offsets=off, offsets=unit)
            _same(got, exp, (name, label, unit))
            calls += 1
            if t and not (off is not None and len(t) == len(rows)):   # (a call that reached the device)
                st = gv.stats()
                what = {k: st[k] for k in ("n_rows", "rows_route", "offsets_unit", "n_ids", "normalize")}
                assert what == dict(n_rows=len(rows), rows_route=1, offsets_unit=UNIT_CODE[unit], n_ids=len(exp[0]),
                                    normalize=c.flags), (name, label, unit, what)
                if guard:
                    assert st["guard_zones"] > 0, (name, label, unit)
                if debug_build:
                    assert st["reserved0"] == 1, "not the bounds-checking build"
    return calls


@pytest.mark.parametrize("name", K.names())
def test_rows_edge(name):
    check_case(name)


def check_pack(max_len, guard=False):
    import torch
    gv = _handle(tuple(K.PLAIN), 0, guard)
    n = 0
    for k, (cls_id, sep_id, docs) in enumerate(K.pack_batches(max_len)):
        label = (max_len, cls_id, sep_id, len(docs))
        ids, splits = [], [0]
        for d in docs:
            ids += K.encode_doc(K.PLAIN, 0, d, "byte")[0]
            splits.append(len(ids))
        want, want_len, cut = R.pack(ids, splits, max_len, cls_id, sep_id, K.PAD)
        n_rows = len(docs)
        got, lens = gv.encode_padded(docs=docs, max_len=max_len, cls_id=cls_id, sep_id=sep_id, pad_id=K.PAD)
        st = gv.stats()
        assert got.dtype == np.int32 and got.shape == (n_rows, max_len) and lens.dtype == np.int32 and lens.shape == (n_rows,), label
        assert lens.tolist() == want_len, (label, "lengths", _first_difference(lens.tolist(), want_len))
        assert got.tolist() == want, (label, "cells", _first_difference(got.tolist(), want))
        assert st["rows_truncated"] == cut and st["n_rows"] == n_rows and st["rows_route"] == 1, (label, st["rows_truncated"], cut)
        # the device form: caller-owned tensors with three rows of sentinels behind n_rows
        text, starts = R.join_docs(docs)
        t = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
        o = torch.tensor(starts, dtype=torch.int64, device="cuda:0") if k % 2 == 0 else None
        own_ids = torch.full((n_rows + 3, max_len), -7, dtype=torch.int32, device="cuda:0")
        own_len = torch.full((n_rows + 3,), -7, dtype=torch.int32, device="cuda:0")
        v_ids, v_len = gv.encode_padded_tensor(t, doc_offsets=o, max_len=max_len, cls_id=cls_id, sep_id=sep_id, pad_id=K.PAD,
                                               out=(own_ids, own_len))
        assert tuple(v_ids.shape) == (n_rows, max_len) and v_ids.data_ptr() == own_ids.data_ptr(), label
        assert own_ids[:n_rows].cpu().tolist() == want and own_len[:n_rows].cpu().tolist() == want_len, (label, "device form")
        assert bool((own_ids[n_rows:] == -7).all()) and bool((own_len[n_rows:] == -7).all()), (label, "rows behind n_rows")
        assert gv.stats()["rows_truncated"] == cut and gv.stats()["n_rows"] == n_rows, (label, "device form")
        n += 1
    return n


@pytest.mark.parametrize("max_len", K.MAX_LENS)
def test_pack_edge(max_len):
    assert check_pack(max_len) == (20 if max_len >= 2 else 15)


# ---- the bounds-checking build and the arena guard --------------------------------------------------------------------------------

def subset_grid(guard=False, debug_build=False, out_json=None):
    """the fixed subset, one representative per family and four lane-group widths; the outcome of each goes to out_json as it
    comes.  An error that is no failed comparison ends the run: nothing is started on the GPU behind it."""
    results = {}
    for name in list(K.SUBSET) + ["P_%d" % m for m in K.SUBSET_MAX_LENS]:
        stop = False
        try:
            if name.startswith("P_"):
                check_pack(int(name[2:]), guard=guard)
            else:
                check_case(name, guard=guard, debug_build=debug_build)
            results[name] = "ok"
        except AssertionError:
            results[name] = traceback.format_exc()[-2000:]
        except Exception:
            results[name] = traceback.format_exc()[-2000:]
            stop = True
        if out_json:
            with open(out_json, "w") as f:
                json.dump(results, f)
        if stop:
            break
    return results


def _run_debug(out_json):
    subset_grid(debug_build=True, out_json=out_json)


def test_rows_edges_arena_guard():
    results = subset_grid(guard=True)
    bad = {n: r for n, r in results.items() if r != "ok"}
    assert not bad and len(results) == len(K.SUBSET) + len(K.SUBSET_MAX_LENS), "\n".join("%s: %s" % kv for kv in sorted(bad.items())[:4])


def test_rows_edges_bounds_build(tmp_path):
    """the subset in the bounds-checking build (line_write_kernel's o <= n_rows and the rebase's s.x >= base are range-checked
    there: kSiteSpan)"""
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    out = tmp_path / "results.json"
    r = R0.run_in_child(tmp_path, "test_gpu_rows_edges", "_run_debug", (str(out),), {"WP_LIB": dbg}, timeout=600, check=False)
    results = {}
    if out.exists():
        with open(str(out)) as f:
            results = json.load(f)
    names = list(K.SUBSET) + ["P_%d" % m for m in K.SUBSET_MAX_LENS]
    tail = "child ended with %d: %s %s" % (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    bad = {n: results.get(n, "not run") for n in names if results.get(n) != "ok"}
    assert not bad and r.returncode == 0 and "CHILD_OK" in r.stdout, "\n".join("%s: %s" % kv for kv in sorted(bad.items())[:4]) + tail
