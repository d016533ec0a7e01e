"""CPU checks of the byte-level BPE layer: the header against the ctypes mirrors and the library's exports, the generated
tables, every argument rule before a device is needed, and tests/bpe_model.py, the contract's executable form, against
`regex` and `tokenizers` where they are installed."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import unicodedata

import numpy as np
import pytest

import bpe_model as M
import wordpiece_amd as W
from wordpiece_amd import bpe as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB, ARG, TOO_LARGE = ["[UNK]", "a", "b"], 6, 2
ALPHABET = list("abcXYZé中文ßΩ") + list("0123٣४²Ⅷ") + list("'''  \t\n\r\x0b\x0c\x1c\x85\xa0 　") + list(".,!-_$€​") + list("stmdrevl")
GPT2 = r"'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"


def test_symbols_structs_and_tables_match_the_header(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "wordpiece_amd_bpe.h")).read()
    assert sorted(re.findall(r"\b(wp_\w+)\s*\(", hdr.split("#ifndef")[1])) == sorted(B.ABI_SYMBOLS)
    assert all(hasattr(B.lib(), name) and name not in W.ABI_SYMBOLS for name in B.ABI_SYMBOLS) and "bpe_load" not in dir(W)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wordpiece_amd_bpe.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(wp_bpe_model), offsetof(wp_bpe_model, n_ids), offsetof(wp_bpe_model, reserved),\n'
                   '         sizeof(wp_bpe_spec), offsetof(wp_bpe_spec, reserved), sizeof(wp_bpe_result), offsetof(wp_bpe_result, n_pieces), sizeof(wp_bpe_stats),\n'
                   '         WP_BPE_SLOTS, WP_BPE_PATTERN_GPT2, WP_BPE_WANT_OFFSETS | WP_BPE_WANT_PIECES);\n  return 0;\n}\n')
    subprocess.run([os.environ.get("CC", "gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "sz"), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "sz")], check=True, capture_output=True, text=True).stdout.split()]
    Mo, P, T, U = B.BpeModel, B.BpeSpec, B.BpeResult, B.BpeStats
    assert got == [C.sizeof(Mo), Mo.n_ids.offset, Mo.reserved.offset, C.sizeof(P), P.reserved.offset, C.sizeof(T), T.n_pieces.offset, C.sizeof(U), B.WP_BPE_SLOTS,
                   B.WP_BPE_PATTERN_GPT2, B.WP_BPE_WANT_OFFSETS | B.WP_BPE_WANT_PIECES]
    assert (C.sizeof(Mo), C.sizeof(P), C.sizeof(T), C.sizeof(U)) == (40, 24, 64, 80)
    spec = importlib.util.spec_from_file_location("gen_bpe_tables", os.path.join(ROOT, "tools", "gen_bpe_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    table = open(os.path.join(ROOT, "wordpiece_amd", "csrc", "bpe_tables.h")).read()
    if '"%s"' % unicodedata.unidata_version in table:  # (another Unicode version generates another table)
        assert gen.render() == table
    assert sorted(gen.SPACES) == sorted(M.SPACES) and len(M.SPACES) == 25


GOOD = dict(n_merges=1, n_ids=257, pattern=0, reserved=0)
BAD_MODELS = [(dict(pattern=1), ARG, b"pattern"), (dict(reserved=1), ARG, b"reserved"), (dict(n_ids=255), ARG, b"n_ids"), (dict(n_ids=2 ** 31), ARG, b"n_ids"),
              (dict(n_merges=-1), ARG, b"n_merges"), (dict(n_merges=2 ** 30), TOO_LARGE, b"n_merges"), (dict(byte_id=None), ARG, b"byte_id is NULL"),
              (dict(merges=None), ARG, b"merges is NULL"), (dict(bytes={7: 300}), ARG, b"byte_id[7] is outside"), (dict(bytes={9: 3}), ARG, b"byte_id[9] is the id of an earlier byte"),
              (dict(triples=[(1, 2, 257)]), ARG, b"merges[0] has an id outside"), (dict(triples=[(1, 2, 256), (1, 2, 256)], n_merges=2), ARG, b"merges[1] repeats the pair of merges[0]"),
              (dict(triples=[(1, 256, 256)]), ARG, b"merges[0] has an operand that is neither"), (dict(triples=[(256, 1, 256), (1, 2, 256)], n_merges=2), ARG, b"merges[0] has an operand"),
              (dict(slot=4), ARG, b"slot"), (dict(slot=-1), ARG, b"slot"), (dict(model=None), ARG, b"m is NULL")]


@pytest.mark.parametrize("fields,code,msg", BAD_MODELS, ids=["%s" % (f,) for f, _, _ in BAD_MODELS])
def test_model_errors_come_before_the_device_and_name_the_field(fields, code, msg):
    """(the improper lists among them: an operand that only a later merge, or none, produces)"""
    v, f = W.Vocab(VOCAB), dict(fields)
    byte_id, triples = np.arange(256, dtype=np.int32), np.array(f.pop("triples", [(1, 2, 256)]), dtype=np.int32)
    for b, i in f.pop("bytes", {}).items():
        byte_id[b] = i
    ptr = dict(byte_id=byte_id.ctypes.data, merges=triples.ctypes.data)
    ptr.update((k, f.pop(k)) for k in list(f) if k in ptr)
    slot, has_model = f.pop("slot", 0), f.pop("model", True)
    m = B.BpeModel(ptr["byte_id"], ptr["merges"], **dict(GOOD, **f))
    assert B.lib().wp_bpe_load(v._h, slot, C.byref(m) if has_model else None) == code
    err = B.lib().wp_last_error()
    assert msg in err and err.startswith(b"bpe: "), err
    assert B.bpe_stats(v)["model_ids"] == 0  # nothing was loaded


def _call(v, spec, device, out=True, data=b"abab", off=(0, 2, 4), n=None):
    """one of the two calls with a result full of garbage (the call clears it) -> (code, result)"""
    o = B.BpeResult(*range(1, 9))
    sp, op = None if spec is None else C.byref(spec), C.byref(o) if out else None
    off = None if off is None else np.asarray(off, dtype=np.int64)
    n = (0 if off is None else len(off) - 1) if n is None else n
    if device:  # (pointers that are never dereferenced: the argument rules come first)
        return B.lib().wp_bpe_encode_rows_device(v._h, C.c_void_p(256), None if off is None else C.c_void_p(512), n, sp, op), o
    return B.lib().wp_bpe_encode_rows(v._h, data, None if off is None else off.ctypes.data, n, sp, op), o


BAD_CALLS = [(dict(spec=None), ARG, b"spec is NULL"), (dict(out=False), ARG, b"out is NULL"), (dict(slot=4), ARG, b"slot"), (dict(slot=-1), ARG, b"slot"),
             (dict(want=4), ARG, b"want has bits outside 3"), (dict(pad=1), ARG, b"pad must be 0"), (dict(pad2=1), ARG, b"pad2"), (dict(reserved=1), ARG, b"reserved"),
             (dict(off=None, n=2), ARG, b"row_off is NULL"), (dict(n=2 ** 31), TOO_LARGE, b"2^31 rows or more"), (dict(slot=1), ARG, b"slot 1 holds no model")]
HOST_ONLY = [(dict(data=None), ARG, b"data is NULL"), (dict(off=(0, 3, 2)), ARG, b"row 1"), (dict(off=(1, 2)), ARG, b"row 0"), (dict(off=(0, 2 ** 32)), TOO_LARGE, b"UINT32_MAX")]


@pytest.mark.parametrize("fields,code,msg", BAD_CALLS + HOST_ONLY, ids=["%s" % (f,) for f, _, _ in BAD_CALLS + HOST_ONLY])
def test_call_errors_come_before_the_device_and_name_the_field(fields, code, msg):
    v, f = W.Vocab(VOCAB), dict(fields)
    how = {k: f.pop(k) for k in list(f) if k in ("out", "data", "off", "n")}
    spec = None if "spec" in f else B.BpeSpec(0, 0, 0, 0, 0)
    for name, x in ({} if spec is None else f).items():
        setattr(spec, name, x)
    for device in ((False,) if (fields, code, msg) in HOST_ONLY else (False, True)):
        rc, o = _call(v, spec, device, **how)
        err = B.lib().wp_last_error()
        assert rc == code and msg in err and err.startswith(b"bpe: "), (device, err)
        assert not how.get("out", True) or not any(getattr(o, k) for k, _ in o._fields_), device
    assert B.bpe_stats(v)["n_rows"] == -1  # none of these was a call


def test_what_needs_no_device():
    v = W.Vocab(VOCAB)
    assert B.bpe_stats(v, 3) == dict(dict.fromkeys([k for k, _ in B.BpeStats._fields_], 0), n_rows=-1)
    B.bpe_clear(v, 2)  # (an empty slot: nothing to free)
    with pytest.raises(W.WordPieceError, match="slot 0 holds no model"):
        B.bpe_encode_rows(v, b"", [0])
    vocab, pairs = M.Model(range(256), [(104, 105, 256)]).vocab()
    with pytest.raises(W.WordPieceError, match="merge 0 .* needs 'hi', which the vocabulary lacks"):
        B.bpe_load(v, {t: i for t, i in vocab.items() if t != "hi"}, pairs)
    with pytest.raises(W.WordPieceError, match="lacks byte 0x00"):
        B.bpe_load(v, {t: i for t, i in vocab.items() if i != 0}, ["h i"])
    assert B.bytes_to_unicode() == M.bytes_to_unicode() and len(set(B.bytes_to_unicode().values())) == 256 and B.bytes_to_unicode()[0x20] == "Ġ"
    assert B.lib().wp_get_bpe_stats(v._h, 4, C.byref(B.BpeStats())) == ARG and b"bpe: slot" in B.lib().wp_last_error()


def test_pinned_pieces_and_merges_of_the_contract():
    cut = lambda s: [s.encode()[a:b].decode() for a, b in M.pieces(s.encode())]  # noqa: E731
    assert cut("Hello  world's we'll 'tis  ") == ["Hello", " ", " world", "'s", " we", "'ll", " '", "tis", "  "]
    assert cut("a's'd x'S 12ab\t b 　c") == ["a", "'s", "'d", " x", "'", "S", " 12", "ab", "\t", " b", " ", "　", "c"]
    assert M.pieces(b"\xc3 \xe4\xb8") == [(0, 1), (1, 4)] and M.pieces(b"\xe4\xb8\xad\xe4\xb8a") == [(0, 3), (3, 5), (5, 6)] and M.pieces(b"") == []
    m = M.Model(range(256), [(97, 97, 256), (256, 97, 257), (256, 256, 258)])
    assert [i for i, _ in m.merge(b"aaa")] == [257] and [i for i, _ in m.merge(b"aaaaa")] == [256, 257] and m.merge(b"aaaa") == [(258, 4)]


def test_the_pieces_against_regex():
    regex = pytest.importorskip("regex")
    rng, pat = np.random.default_rng(5), regex.compile(GPT2)
    for _ in range(3000):
        s = "".join(rng.choice(ALPHABET, size=int(rng.integers(0, 24))))
        assert [s.encode()[a:b].decode() for a, b in M.pieces(s.encode())] == pat.findall(s), repr(s)


def test_ids_and_offsets_against_tokenizers():
    tk = pytest.importorskip("tokenizers")
    rng = np.random.default_rng(9)
    texts = ["".join(rng.choice(ALPHABET, size=40)) for _ in range(300)] + ["the cat's hat isn't that flat, we'll see 1234 cats  " * 3]
    m = M.train([t.encode() for t in texts[::2]], 150, seed=2)
    vocab, pairs = m.vocab()
    hf = tk.Tokenizer(tk.models.BPE(vocab=vocab, merges=pairs))
    hf.pre_tokenizer = tk.pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
    for t in texts:
        enc, got = hf.encode(t), m.encode([t.encode()])
        assert enc.ids == got["ids"].tolist(), repr(t)
        if t.isascii():  # (the package counts characters, the contract bytes)
            assert [list(o) for o in enc.offsets] == np.stack([got["begin"], got["end"]], axis=1).tolist(), repr(t)
    assert got["rounds"] >= 2 and len(m.merges) == 150
