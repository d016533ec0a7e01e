"""GPU tests (-m gpu) of the UTF-8 decode stage at its word, lane, row, wave and tile edges (csrc/decode.h: dec_load_rows,
decode_count_kernel, decode_write_kernel and its aligned flush; the same row loads in csrc/offsets.h and csrc/normalize.h),
on the inputs of decode_cases.py.  Every case of groups B (straddles), E (ends), A (alignment of the ASCII flush), U (4-byte
symbols) and M (alphabet marking), on fresh handles:

  - default handle: the ids equal the CPU oracle's; wp_stats.n_text and .alphabet equal the layout model's; the
    invalid-unicode warning is on stderr exactly when the model says a byte is dropped (the valid tile-straddling B cases
    pin the wrap-and-cancel of decode_count_kernel's byte accounting);
  - WP_OPT_KEEP_DEBUG handle: debug fetch 6 equals the code points, fetch 0 the rank-plus-one symbols over the first n_text
    positions, fetch 7 the class bits (space, spacing, punctuation from the oracle's predicates, soft from the vocabulary);
  - encode_with_offsets in both units equals offsets_model (the byte unit is what checks cp_byte_kernel's lead positions);
  - fast_encode equals the oracle's fast ids where the fast entry point applies;
  - normalize(flags=0) equals the UTF-8 of the model's code points, and WP_NORM_BERT_UNCASED equals normalize_model (B, E, and
    M_ascii_flags: all 128 ASCII values x 9);
  - the same text again on the same handle behind a text of another group: same ids, same n_text.

Group P runs the _device entry points (Linear, offsets, fast, normalise, the lines mode of the rows call) directly on a
buffer that holds the text and 64 dirty bytes behind nbytes, and expects what the host entry points give for the bare text;
an unaligned device pointer is an argument error.  Group H encodes a text that ends in a cut-off lead behind one that has
continuation bytes at the same place, on one handle.  B, E, A, U and M run once more on the default handle in the
bounds-checking build with guard zones (a child process).

Wall time of this file on an MI355X machine: 26 s for its 269 tests (1,641 cases; the bounds-build child 6 s of it).  The whole
-m gpu suite has still not been timed in one job on the same machine (see the note in test_gpu_walk_edges.py).

Register-only mutations of the decoder, each run once against groups B and E on a scratch build: w[r][4] of lane 63 taken from
the shuffle failed the valid and accepted B cases at the row, wave and tile boundaries (48) and the E lengths one to three
bytes past a row, wave or tile end that end in a complete sequence; tail = 0 failed the same B cases at the wave and tile
boundaries (32) and those E lengths past a wave or tile end; utf8_starts without bad3 failed the ten B_*_rej_E09F /
B_*_rej_EDA0 cases.  No case failed on the unmutated kernels."""
import ctypes as C
import functools
import json
import os
import traceback

import numpy as np
import pytest
import torch

import decode_cases as D
import normalize_model as NM
import offsets_model as OM
import oracle_lib as O
import round0_cases as R
import wordpiece_amd as W

pytestmark = pytest.mark.gpu
PKG = os.path.dirname(os.path.abspath(W.__file__))
CLS_SPACE, CLS_SPACING, CLS_SOFT, CLS_PUNCT = 1, 2, 4, 8   # common.h, kCls*
CLASS_MASK = CLS_SPACE | CLS_SPACING | CLS_SOFT | CLS_PUNCT  # (the anchor kernels add kClsWordPrefix / kClsAnchor above them)
WARNING = "Input contains invalid unicode characters"
WP_ERR_ARG = 6


def class_bits(cps, soft):
    L = O.lib()
    table = {c: (CLS_SPACE if L.wpo_is_space(c) else 0) | (CLS_SPACING if L.wpo_is_spacing_char(c) else 0) |
             (CLS_PUNCT if L.wpo_is_punctuation(c) else 0) | (CLS_SOFT if c in soft else 0) for c in set(cps)}
    return np.array([table[c] for c in cps], dtype=np.int32)


@functools.lru_cache(maxsize=2)
def reference(name, light=False):
    """everything the checks of one case compare against, computed once (light: what the default handle's ids, n_text and
    alphabet need)"""
    text, vocab, expect = D.build(name)
    m = D.Layout(text, vocab)
    ov = O.Vocab(vocab)
    ref = dict(text=text, vocab=vocab, expect=expect, m=m, ids=ov.encode(text))
    if light:
        return ref
    ids_m, spans, t, starts = OM.encode_spans(text, vocab)
    assert ids_m == ref["ids"].tolist() and t == m.cps, name
    ref["char"] = np.array(spans, dtype=np.int64).reshape(-1, 2)
    ref["byte"] = np.array(OM.to_bytes(spans, text, starts), dtype=np.int64).reshape(-1, 2)
    ref["fast"] = ov.fast_encode(text) if expect["fast"] else None
    ref["cps"] = np.array(m.cps, dtype=np.int32)
    ref["sym"] = np.array(m.symbols(), dtype=np.int32)
    ref["cls"] = class_bits(m.cps, D.soft_set(vocab))
    ref["norm0"] = "".join(map(chr, m.cps)).encode("utf8")
    ref["norm7"] = NM.normalize(text, W.WP_NORM_BERT_UNCASED)[0] if name[0] in "BE" or name == "M_ascii_flags" else None
    return ref


@functools.lru_cache(maxsize=None)
def _between(group, vocab):
    """the text encoded between the two encodes of a case, of another group, and its ids with the case's vocabulary"""
    other = D.build("B_tile_L4s1_valid" if group in "AU" else "A_a3")[0]
    return other, O.Vocab(list(vocab)).encode(other)


def _encode_watching_stderr(gv, text, capfd):
    if capfd is None:
        return gv.encode(text), None
    capfd.readouterr()
    ids = gv.encode(text)
    return ids, WARNING in capfd.readouterr().err


def check_default_handle(name, ref, capfd=None, debug_build=False):
    text, vocab, m = ref["text"], ref["vocab"], ref["m"]
    gv = W.Vocab(vocab)
    ids, warned = _encode_watching_stderr(gv, text, capfd)
    st = gv.stats()
    print(name, len(text), {k: st[k] for k in ("n_text", "alphabet", "vocab_in_s", "symbol_bits")}, "warned", warned, flush=True)
    assert np.array_equal(ids, ref["ids"]), (name, "ids")
    assert st["n_text"] == m.n_text, (name, "n_text", st["n_text"], m.n_text)
    assert st["alphabet"] == m.alphabet, (name, "alphabet", st["alphabet"], m.alphabet)
    if capfd is not None:
        assert warned == m.dropped, (name, "the invalid-unicode warning", warned, m.dropped)
    if "vocab_in_s" in ref["expect"]["claims"]:
        assert st["vocab_in_s"] == ref["expect"]["claims"]["vocab_in_s"], (name, "vocab_in_s")
    if debug_build:
        assert st["reserved0"] == 1 and st["guard_zones"] > 0, "not the bounds-checking build with guard zones"
    return gv


def check_case(name, capfd=None):
    ref = reference(name)
    text, vocab, m = ref["text"], ref["vocab"], ref["m"]
    gv = check_default_handle(name, ref, capfd)
    # ---- offsets in both units, the fast path, the normalise kernels: the same row loads and lead masks again
    for unit in ("char", "byte"):
        ids_o, offs = gv.encode_with_offsets(text, unit)
        assert np.array_equal(np.array(ids_o), ref["ids"]), (name, unit, "ids of the offsets call")
        assert np.array_equal(np.array(offs, dtype=np.int64).reshape(-1, 2), ref[unit]), (name, unit, "offsets")
    if ref["fast"] is not None:
        assert np.array_equal(gv.fast_encode(text), ref["fast"]), (name, "fast ids")
    assert gv.normalize(text, flags=0) == ref["norm0"], (name, "normalize, no flags")
    if ref["norm7"] is not None:
        assert gv.normalize(text, flags=W.WP_NORM_BERT_UNCASED) == ref["norm7"], (name, "normalize, BERT uncased")
    # ---- the same handle again, a text of another group in between
    other, other_ids = _between(name[0], tuple(vocab))
    assert np.array_equal(gv.encode(other), other_ids), (name, "text in between")
    assert np.array_equal(gv.encode(text), ref["ids"]) and gv.stats()["n_text"] == m.n_text, (name, "encode behind another text")
    # ---- what the decoder wrote, position by position
    gd = W.Vocab(vocab)
    gd.set_option(W.WP_OPT_KEEP_DEBUG, 1)
    assert np.array_equal(gd.encode(text), ref["ids"]), (name, "ids, debug handle")
    st = gd.stats()
    assert st["n_text"] == m.n_text, (name, "n_text, debug handle")
    cap = max(int(st["n_total"]), 1)
    assert np.array_equal(gd.debug_fetch(6, cap), ref["cps"]), (name, "code points (fetch 6)")
    assert np.array_equal(gd.debug_fetch(0, cap)[:m.n_text], ref["sym"]), (name, "dense symbols (fetch 0)")
    assert np.array_equal(gd.debug_fetch(7, cap) & CLASS_MASK, ref["cls"]), (name, "class bits (fetch 7)")


def check_block(names, capfd):
    """several cases in one test: every failed comparison is reported, by case; any other error ends the test at once"""
    failed = {}
    for name in names:
        try:
            check_case(name, capfd)
        except AssertionError as e:
            failed[name] = str(e)[:300]
    assert not failed, "%d of %d cases failed: %s" % (len(failed), len(names), json.dumps(failed, indent=1)[:6000])


@pytest.mark.parametrize("name", D.names("BAUM"))
def test_decode_edge(name, capfd):
    check_case(name, capfd)


E_BLOCKS = 32


@pytest.mark.parametrize("block", range(E_BLOCKS))
def test_decode_end_block(block, capfd):
    """group E, about twenty lengths x kinds of end per test (most of them a few bytes long)"""
    check_block(D.names("E")[block::E_BLOCKS], capfd)


# ---- group P: the bytes behind nbytes are ignored -------------------------------------------------------------------------------

def _device_text(text, tail=b""):
    """a device buffer that holds text + tail (zeros behind), 4-byte aligned, readable to the next multiple of 16 behind
    the text"""
    n = len(text) + len(tail)
    buf = torch.zeros((len(text) + 15) // 16 * 16 + len(tail) + 16, dtype=torch.uint8, device="cuda")
    buf[:n] = torch.frombuffer(bytearray(text + tail), dtype=torch.uint8).to("cuda")
    torch.cuda.synchronize()
    assert buf.data_ptr() % 4 == 0
    return buf


def _host_copy(ptr, n, typestr="<i4", cols=0):
    if not n:
        return np.zeros((0, cols) if cols else 0, dtype=np.dtype(typestr))
    return torch.as_tensor(W.DeviceIds(ptr, n, cols=cols, typestr=typestr), device="cuda").cpu().numpy().copy()


def device_calls(gv, ptr, nbytes):
    """the five _device entry points on the text at ptr -> their results on the host, or (rc, message) where one fails"""
    L, out = W.lib(), {}
    vp, sz = C.c_void_p, C.c_size_t

    def run(key, call, fetch):
        rc = call()
        out[key] = fetch() if rc == 0 else (rc, L.wp_last_error().decode())

    d_ids, d_offs, d_splits, d_out, n, rows = vp(), vp(), vp(), vp(), sz(), sz()
    run("linear", lambda: L.wp_linear_encode_device(gv._h, vp(ptr), nbytes, C.byref(d_ids), C.byref(n)),
        lambda: _host_copy(d_ids.value, n.value))
    run("offsets", lambda: L.wp_linear_encode_offsets_device(gv._h, vp(ptr), nbytes, W.WP_OFFSETS_BYTES, C.byref(d_ids), C.byref(d_offs),
                                                             C.byref(n)),
        lambda: (_host_copy(d_ids.value, n.value), _host_copy(d_offs.value, n.value, cols=2).astype(np.int64)))
    run("fast", lambda: L.wp_fast_encode_device(gv._h, vp(ptr), nbytes, C.byref(d_ids), C.byref(n)),
        lambda: _host_copy(d_ids.value, n.value))
    run("normalize", lambda: L.wp_normalize_device(gv._h, vp(ptr), nbytes, W.WP_NORM_BERT_UNCASED, C.byref(d_out), C.byref(n)),
        lambda: _host_copy(d_out.value, n.value, "|u1").tobytes())
    run("rows", lambda: L.wp_linear_encode_rows_device(gv._h, vp(ptr), nbytes, None, 0, -1, C.byref(d_ids), C.byref(d_splits),
                                                       C.byref(d_offs), C.byref(n), C.byref(rows)),
        lambda: (_host_copy(d_ids.value, n.value), _host_copy(d_splits.value, rows.value + 1, "<i8")))
    return out


def host_calls(gv, text):
    ids_o, offs = gv.encode_with_offsets(text, "byte")
    ids_r, splits = gv.encode_rows(text=text)
    return {"linear": gv.encode(text), "offsets": (np.array(ids_o), np.array(offs, dtype=np.int64).reshape(-1, 2)),
            "fast": gv.fast_encode(text), "normalize": gv.normalize(text, flags=W.WP_NORM_BERT_UNCASED),
            "rows": (np.array(ids_r), np.array(splits))}


def _same(a, b):
    if isinstance(a, tuple):
        return isinstance(b, tuple) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, bytes):
        return a == b
    return isinstance(b, np.ndarray) and np.array_equal(a, b)


P_BLOCKS = 16


@pytest.mark.parametrize("block", range(P_BLOCKS))
def test_bytes_behind_the_text_are_ignored(block):
    """the _device entry points on text + dirty tail equal the host entry points on the bare text (ids, offsets, fast ids,
    normalised bytes, and ids and row splits of the lines mode: one more line end behind nbytes would be one more row)"""
    gv = W.Vocab(D.BASE)
    failed = {}
    for name in D.names("P")[block::P_BLOCKS]:
        text, _, expect = D.build(name)
        want = host_calls(gv, text)
        assert np.array_equal(want["linear"], O.Vocab(D.BASE).encode(text)), name
        buf = _device_text(text, expect["tail"])
        got = device_calls(gv, buf.data_ptr(), len(text))
        bad = [k for k in want if not _same(want[k], got[k])]
        if bad:
            failed[name] = bad
    assert not failed, failed


def test_unaligned_device_text_is_an_argument_error():
    text = D.build("E_len37_ascii")[0]
    buf = _device_text(b"a" + text)
    gv = W.Vocab(D.BASE)
    before = gv.stats()
    for shift in (1, 2, 3):
        got = device_calls(gv, buf.data_ptr() + shift, len(text) - 3)
        for key, res in got.items():
            assert isinstance(res, tuple) and res[0] == WP_ERR_ARG and "4-byte aligned" in str(res[1]), (shift, key, res)
    assert gv.stats() == before, "no encode ran on the handle"


# ---- group H: one handle, a cut-off lead where the text before had continuation bytes ------------------------------------------------

@pytest.mark.parametrize("name", D.names("H"))
def test_cut_off_lead_behind_continuation_bytes(name):
    second, vocab, expect = D.build(name)
    first = expect["first"]
    ov, m = O.Vocab(vocab), D.Layout(second, vocab)
    gv = W.Vocab(vocab)
    for text in (first, second):
        assert np.array_equal(gv.encode(text), ov.encode(text)), (name, len(text), "ids")
    assert gv.stats()["n_text"] == m.n_text, (name, "n_text")
    for text in (first, second):
        assert np.array_equal(gv.fast_encode(text), ov.fast_encode(text)), (name, len(text), "fast ids")
    assert gv.stats()["n_text"] == m.n_text, (name, "n_text, fast")
    for text in (first, second):
        ids, offs = gv.encode_with_offsets(text, "byte")
        ids_m, offs_m = OM.encode_with_offsets(text, vocab, "byte")
        assert np.array(ids).tolist() == ids_m and np.array(offs, dtype=np.int64).reshape(-1, 2).tolist() == [list(x) for x in offs_m], \
            (name, len(text), "offsets")
    assert gv.normalize(first, flags=0) == "".join(map(chr, D.Layout(first).cps)).encode("utf8")
    assert gv.normalize(second, flags=0) == "".join(map(chr, m.cps)).encode("utf8"), (name, "normalize")


# ---- the bounds-checking build with guard zones -------------------------------------------------------------------------------------

def _run_debug(out_json):
    """(in a child process on libwordpiece_amd_dbg.so with WP_ARENA_GUARD=1) every case of B, E, A, U and M on the default
    handle; the outcome of each goes to out_json as it comes.  An error that is no failed comparison ends the run: nothing
    is started on the GPU behind it."""
    results = {}
    for name in D.names():
        stop = False
        try:
            check_default_handle(name, reference(name, True), debug_build=True)
            results[name] = "ok"
        except AssertionError:
            results[name] = traceback.format_exc()[-2000:]
        except Exception:
            results[name] = traceback.format_exc()[-2000:]
            stop = True
        with open(out_json, "w") as f:
            json.dump(results, f)
        if stop:
            return


def test_decode_edges_bounds_build(tmp_path):
    """Groups B, E, A, U and M in the bounds-checking build with a guard zone behind every arena allocation: a symbol, class
    byte or code point stored past the end of its array (the flush's spill bytes, the 16-byte stores of the 4-byte symbols)
    makes the encode fail."""
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    out = tmp_path / "results.json"
    r = R.run_in_child(tmp_path, "test_gpu_decode_edges", "_run_debug", (str(out),), {"WP_LIB": dbg, "WP_ARENA_GUARD": "1"},
                       timeout=900, check=False)
    results = {}
    if out.exists():
        with open(str(out)) as f:
            results = json.load(f)
    tail = "child ended with %d: %s %s" % (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    bad = {n: results.get(n, "not run") for n in D.names() if results.get(n) != "ok"}
    assert not bad and r.returncode == 0 and "CHILD_OK" in r.stdout, "\n".join("%s: %s" % kv for kv in sorted(bad.items())[:4]) + tail
