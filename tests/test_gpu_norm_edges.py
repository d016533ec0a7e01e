"""GPU tests (-m gpu) of the normalise pre-pass at its path, row, flush and map edges (csrc/normalize.h: norm_count_kernel,
norm_write_kernel, norm_flush_row, span_source_kernel; the word-wide ASCII helpers of csrc/utf8_swar.h; the tables'
device copies), on the inputs of norm_cases.py.  All comparisons are exact; the reference is normalize_model (the rule over
unicodedata) and offsets_model.

  - every case of A (every ASCII value through each of the four paths), X (rows that give 0..8 bytes, the most, nothing),
    S (a code point across a seam, under the rule) and F (100 compositions), under every flag set 0..7: Vocab.normalize
    equals the model's bytes; a failure names the first differing byte, its row, its lane and the path the layout model
    gives for it.  normalize_tensor does the same under flags 1 and 7 on a device buffer that holds 64 non-zero bytes
    behind nbytes, at a 4-aligned length and at one that is not;
  - M, and A, X, S under flags 1, 4, 7, on handles built with normalize=f and the case's single-symbol vocabulary: the ids
    equal the plain handle's ids of the model-normalised text, encode_with_offsets in both units equals
    normalize_model's spans carried back, stats()["norm_bytes"] is the model's length, fast_encode agrees;
  - T: every scalar value U+0000..U+10FFFF in order, behind 0..3 ASCII bytes, under every flag set, against the
    expectation built from normalize_model.normalize_cp: the three device copies of the tables as a whole; a mismatch
    names the first code point that differs;
  - H: sequences of calls on one handle, every call against a fresh handle's result (and the model where it applies); the
    shard rule of encode_multi for U+000B / U+000C;
  - A, X, S and M once more in the bounds-checking build with guard zones (a child process): the pre-pass under flags 2 and
    7, the map under flags 7;
  - one case of each of A, X, S, M in the middle and at the end of 2.4 MB of English words, on a normalize=7 handle.

Wall time on an MI355X machine, the -m gpu suite run in two halves of one session with per-test times: this file 42 s for
its 101 tests (510 cases and the four T texts; the bounds-build child 9 s of it; 41.0 s summed over its tests), the other
24 files of the suite 1,063 s summed over their 1,604 tests: 3.9 % on top, under the tenth aimed at, so group F keeps its
100 compositions and T its shifted variants under every flag set.

Found by this file: nothing.  Every comparison held on the kernels as they were; no kernel was changed."""
import functools
import json
import os
import traceback

import numpy as np
import pytest
import torch

import norm_cases as N
import normalize_model as NM
import offsets_model as OM
import round0_cases as R
import wordpiece_amd as W
from test_normalize_tables import _same_unicode
from wordpiece_amd import synth

pytestmark = pytest.mark.gpu
PKG = os.path.dirname(os.path.abspath(W.__file__))
DIRTY = b"\xbf" * 32 + b"Q\x01\xe4\xb8" * 8   # 64 non-zero bytes behind nbytes: continuation bytes, then text


@functools.lru_cache(maxsize=None)
def _plain():
    return W.Vocab(["[UNK]", "a", "##a"])


@functools.lru_cache(maxsize=64)
def _handle(vocab, flags):
    return W.Vocab(list(vocab), normalize=flags)


def _first_difference(text, flags, got, want):
    k = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    return "%d bytes, expected %d; first difference: %s; got %s, expected %s" % (
        len(got), len(want), N.describe(text, flags, k), got[k:k + 8].hex(), want[k:k + 8].hex())


def _device_text(text):
    """a device buffer that holds the text, DIRTY behind it and zeros behind that; readable to the next multiple of 16"""
    buf = torch.zeros((len(text) + len(DIRTY) + 31) // 16 * 16, dtype=torch.uint8, device="cuda")
    buf[:len(text) + len(DIRTY)] = torch.frombuffer(bytearray(text + DIRTY), dtype=torch.uint8).to("cuda")
    assert buf.data_ptr() % 4 == 0
    return buf


def check_pre_pass(name, flag_sets=N.ALL_FLAGS, tensor_flags=(1, 7)):
    """-> the comparisons that failed, as messages"""
    text, _ = N.build(name)
    gv, failed = _plain(), []
    for f in flag_sets:
        want = N.model(text, f)[0]
        got = gv.normalize(text, flags=f)
        if got != want:
            failed.append("%s flags %d: %s" % (name, f, _first_difference(text, f, got, want)))
    if tensor_flags and len(text) > 4:
        buf = _device_text(text)
        n4 = len(text) // 4 * 4
        for n in (n4, n4 - 1):   # the device entry point on the buffer as it stands; through an aligned, zero-padded copy
            for f in tensor_flags:
                want = N.model(text[:n], f)[0]
                got = gv.normalize_tensor(buf[:n], flags=f).cpu().numpy().tobytes()
                if got != want:
                    failed.append("%s flags %d, tensor of %d bytes: %s" % (name, f, n, _first_difference(text[:n], f, got, want)))
    return failed


def check_map(name, flag_sets=N.MAP_FLAGS, fast=True, debug_build=False):
    text, expect = N.build(name)
    failed = []
    for f in flag_sets:
        vocab = expect["claims"].get("vocab") or N.single_symbol_vocab(text, f)
        norm, src_byte, src_cp = N.model(text, f)
        ids_m, spans, _, _ = OM.encode_spans(norm, vocab)
        plain, gv = _handle(tuple(vocab), 0), _handle(tuple(vocab), f)
        want_ids = plain.encode(norm)
        if want_ids.tolist() != ids_m:
            failed.append("%s flags %d: the plain handle's ids of the normalised text differ from the model's" % (name, f))
        ids = gv.encode(text)
        st = gv.stats()
        if debug_build and len(norm):   # (a text that gives nothing: the encode ends behind the pre-pass, without arenas)
            assert st["reserved0"] == 1 and st["guard_zones"] > 0, "not the bounds-checking build with guard zones"
        if not np.array_equal(ids, want_ids):
            failed.append("%s flags %d: ids (%d, expected %d)" % (name, f, len(ids), len(want_ids)))
        if st["norm_bytes"] != len(norm):
            failed.append("%s flags %d: norm_bytes %d, expected %d" % (name, f, st["norm_bytes"], len(norm)))
        for unit in ("char", "byte"):
            want = np.array(NM.carry_spans(spans, text, src_byte, src_cp, unit), dtype=np.int64).reshape(-1, 2)
            ids_o, offs = gv.encode_with_offsets(text, unit)
            offs = np.array(offs, dtype=np.int64).reshape(-1, 2)
            if not np.array_equal(np.array(ids_o), want_ids) or not np.array_equal(offs, want):
                k = next((i for i in range(min(len(offs), len(want))) if tuple(offs[i]) != tuple(want[i])), min(len(offs), len(want)))
                failed.append("%s flags %d, %s offsets: %d spans, expected %d; first difference at id %d: %s, expected %s" % (
                    name, f, unit, len(offs), len(want), k, offs[k:k + 2].tolist(), want[k:k + 2].tolist()))
        if fast and not np.array_equal(gv.fast_encode(text), plain.fast_encode(norm)):
            failed.append("%s flags %d: fast ids" % (name, f))
    return failed


def _report(failed, n):
    assert not failed, "%d comparisons of %d cases failed:\n%s" % (len(failed), n, "\n".join(failed)[:6000])


# ---- the pre-pass alone: A, X, S, F under every flag set ------------------------------------------------------------------------

@pytest.mark.parametrize("name", N.names("A"))
def test_every_ascii_value_through_each_path(name):
    _same_unicode()
    _report(check_pre_pass(name), 1)


BLOCKS = {"X": 6, "S": 12, "F": 6}


@pytest.mark.parametrize("group,block", [(g, b) for g, n in BLOCKS.items() for b in range(n)])
def test_pre_pass_at_row_and_seam_edges(group, block):
    """groups X, S and F, a block of names per test; every failed comparison is reported, any other error ends the test"""
    _same_unicode()
    names = N.names(group)[block::BLOCKS[group]]
    _report([m for name in names for m in check_pre_pass(name)], len(names))


# ---- the source map: M, and A, X, S under flags 1, 4, 7 -------------------------------------------------------------------------

@pytest.mark.parametrize("name", N.names("M") + N.names("A"))
def test_source_map(name):
    _same_unicode()
    _report(check_map(name), 1)


MAP_BLOCKS = {"X": 6, "S": 12}


@pytest.mark.parametrize("group,block", [(g, b) for g, n in MAP_BLOCKS.items() for b in range(n)])
def test_source_map_at_row_and_seam_edges(group, block):
    _same_unicode()
    names = N.names(group)[block::MAP_BLOCKS[group]]
    _report([m for name in names for m in check_map(name)], len(names))


# ---- T: the whole code space ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _t_text():
    return N.t_text(0)


@pytest.mark.parametrize("flags", N.ALL_FLAGS)
def test_whole_code_space(flags):
    """every scalar value through norm_cp's device form and the uploaded tables, at every word phase"""
    _same_unicode()
    images = N.t_images(flags)
    want = b"".join(images)
    gv = _plain()
    for shift in N.T_SHIFTS:
        got = gv.normalize(b"x" * shift + _t_text(), flags=flags)
        if got != b"x" * shift + want:
            raise AssertionError("flags %d, behind %d ASCII bytes: %s" % (flags, shift, N.t_first_difference(got, images, shift)))


# ---- H: one handle, several calls ---------------------------------------------------------------------------------------------------

def _call(gv, call, text, flags):
    if call == "normalize":
        return gv.normalize(text, flags=flags)
    gv.set_option(W.WP_OPT_NORMALIZE, flags)
    if call == "encode":
        return gv.encode(text).tolist()
    ids, offs = gv.encode_with_offsets(text, "byte")
    return np.array(ids).tolist(), np.array(offs).tolist()


@pytest.mark.parametrize("name", sorted(N.SEQUENCES))
def test_calls_on_one_handle(name):
    _same_unicode()
    gv = W.Vocab(N.H_VOCAB)
    for step, (call, text, flags) in enumerate(N.SEQUENCES[name]()):
        got = _call(gv, call, text, flags)
        assert got == _call(W.Vocab(N.H_VOCAB), call, text, flags), (name, step, call, flags, "differs from a fresh handle's")
        if call == "normalize":
            assert got == N.model(text, flags)[0], (name, step, flags, _first_difference(text, flags, got, N.model(text, flags)[0]))
        else:
            want = len(N.model(text, flags)[0]) if flags else 0   # (no flags: the pre-pass does not run)
            assert gv.stats()["norm_bytes"] == want, (name, step, call, flags, "norm_bytes")


@pytest.mark.parametrize("flags", (1, 7, 2, 4))
def test_shards_are_not_cut_at_a_dropped_blank(flags):
    """encode_multi: U+000B and U+000C are blanks only where WP_NORM_CLEAN does not drop them"""
    _same_unicode()
    text = N.shard_text()
    gv = W.Vocab(N.H_SHARD_VOCAB, normalize=flags)
    want = W.Vocab(N.H_SHARD_VOCAB).encode(N.model(text, flags)[0])
    assert want.tolist() == OM.encode_spans(N.model(text, flags)[0], N.H_SHARD_VOCAB)[0]
    assert np.array_equal(gv.encode(text), want), flags
    assert np.array_equal(gv.encode_multi(text, devices=[0, 0]), want), flags


# ---- the bounds-checking build with guard zones -------------------------------------------------------------------------------------

def _run_debug(out_json):
    """(in a child process on libwordpiece_amd_dbg.so with WP_ARENA_GUARD=1) every case of A, X, S and M; the outcome of each
    goes to out_json as it comes.  An error that is no failed comparison ends the run: nothing is started on the GPU
    behind it."""
    results = {}
    for name in N.names("AXSM"):
        stop = False
        try:
            failed = check_map(name, flag_sets=(7,), fast=False, debug_build=True)
            if name[0] != "M":
                failed += check_pre_pass(name, flag_sets=(2, 7), tensor_flags=())
            results[name] = "ok" if not failed else "\n".join(failed)[:2000]
        except AssertionError:
            results[name] = traceback.format_exc()[-2000:]
        except Exception:
            results[name] = traceback.format_exc()[-2000:]
            stop = True
        with open(out_json, "w") as f:
            json.dump(results, f)
        if stop:
            return


def test_norm_edges_bounds_build(tmp_path):
    """A, X, S and M in the bounds-checking build with a guard zone behind every arena allocation: a map entry or a flushed
    dword written past the end of its array makes the call fail."""
    _same_unicode()
    dbg = os.path.join(PKG, "libwordpiece_amd_dbg.so")
    assert os.path.exists(dbg), "run `python -m wordpiece_amd.build`"
    out = tmp_path / "results.json"
    r = R.run_in_child(tmp_path, "test_gpu_norm_edges", "_run_debug", (str(out),), {"WP_LIB": dbg, "WP_ARENA_GUARD": "1"},
                       timeout=900, check=False)
    results = {}
    if out.exists():
        with open(str(out)) as f:
            results = json.load(f)
    tail = "child ended with %d: %s %s" % (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    bad = {n: results.get(n, "not run") for n in N.names("AXSM") if results.get(n) != "ok"}
    assert not bad and r.returncode == 0 and "CHILD_OK" in r.stdout, "\n".join("%s: %s" % kv for kv in sorted(bad.items())[:4]) + tail


# ---- the same inputs inside a text above kRadixSmallN -------------------------------------------------------------------------------
EMBEDDED = ("A_lean_kept", "X_hangul_a3", "S_tile_s1_note_ctrl", "M_probe_first_row_of_tile_2")


@functools.lru_cache(maxsize=None)
def _corpus():
    """2.4 MB of English words cut at a blank in the middle, the vocabulary, and the model-normalised halves (the rule is
    per code point: the normalised text of a concatenation of valid texts is the concatenation of theirs)"""
    text, vocab = synth.english_corpus(2_400_000, seed=5, vocab_size=3000)
    half = text.index(b" ", len(text) // 2)
    a, b = text[:half], text[half + 1:]
    return a, b, [w if isinstance(w, str) else w.decode() for w in vocab], N.model(a, 7)[0], N.model(b, 7)[0]


@pytest.mark.parametrize("name", EMBEDDED)
def test_norm_edge_embedded_at_size(name):
    _same_unicode()
    case, _ = N.build(name)
    case.decode("utf8")   # (valid UTF-8: the model's text of the whole is the concatenation of the parts')
    a, b, words, norm_a, norm_b = _corpus()
    vocab = words + [w for w in N.single_symbol_vocab(case, 7) if w not in set(words)]
    text = a + b" " + case + b" " + b + b" " + case
    norm_case = N.model(b" " + case + b" ", 7)[0]
    norm = norm_a + norm_case + norm_b + norm_case[:-1]
    gv = W.Vocab(vocab, normalize=7)
    ids = gv.encode(text)
    st = gv.stats()
    print(name, {k: st[k] for k in ("n_total", "n_bytes", "norm_bytes", "round0_keys_only")}, flush=True)
    assert st["n_total"] > R.RADIX_SMALL_N and st["norm_bytes"] == len(norm), (st["norm_bytes"], len(norm))
    assert np.array_equal(ids, W.Vocab(vocab).encode(norm)), name
