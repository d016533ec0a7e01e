"""CPU tests of the inputs behind test_gpu_decode_edges.py (decode_cases.py): the layout constants are the ones the groups
were laid out for; the layout model reproduces what every builder claims to have built (the lead s bytes in front of the
named boundary, which rows are pure-ASCII rows and at which output alignment, dropped bytes, the number of code points,
the used set); and the references agree with each other on exactly these inputs: the oracle's decoder (code points and
invalid flag), bruteforce.decode, offsets_model.decode_with_starts and, where oracle/_ref was built, the reference's own
decoder; the oracle's ids with offsets_model.encode_spans, the oracle's fast ids with the Python model of
test_oracle_fast.py."""
import collections
import ctypes as C
import os

import pytest

import bruteforce
import decode_cases as D
import offsets_model as OM
import oracle_lib as O
from test_oracle_fast import fast_model


def test_constants_are_read_from_the_headers():
    assert (D.DEC_CHUNK, D.DEC_ROWS, D.LANES, D.BLOCK) == (16, 4, 64, 256), \
        "a constant of the decode layout changed: the cases moved with it — check GROUP_SIZES and update this line"
    assert (D.WORD, D.CHUNK, D.ROW, D.WAVE, D.TILE) == (4, 16, 1024, 4096, 16384)
    assert {k: D.boundary_kind(x) for k, x in D.BOUNDARIES.items()} == {k: k for k in D.BOUNDARIES}


def test_case_count_per_group():
    count = collections.Counter(n[0] for n in D.CASES)
    assert dict(count) == D.GROUP_SIZES and set(count) == set(D.GROUPS)
    # B: every boundary kind x (L, s) placement valid and cut short, every rejected form, every accepted neighbour, the four last bytes
    for kind in D.BOUNDARIES:
        for L in (2, 3, 4):
            for s in range(1, L):
                assert {"B_%s_L%ds%d_%s" % (kind, L, s, v) for v in ("valid", "missing")} <= set(D.CASES)
        assert sum(1 for n in D.CASES if n.startswith("B_%s_" % kind)) == 30
    # P: a 4-byte aligned pointer, nbytes over every residue mod 16, with each kind of end
    for kind in ("ascii", "cut1", "cut2", "cut3"):
        assert {D.build(n)[2]["claims"]["nbytes"] % 16 for n in D.names("P") if "_%s_" % kind in n} == set(range(16)), kind
    assert {int(n.split("_")[1][3:]) for n in D.names("E") if n.startswith("E_len")} == set(D.E_LENGTHS)


def test_layout_model_on_hand_made_texts():
    """the model itself, on texts small enough to check by eye"""
    m = D.Layout(b"a\xd0\xb6b\xe4\xb8", ["a", "##c"])
    assert (m.cps, m.starts, m.dropped, m.n_text) == ([97, 0x436, 98], [0, 1, 3], True, 3)
    assert m.used == {1, 97, 98, 99, 0x436} and m.symbols() == [2, 5, 3] and m.alphabet == 5
    assert m.rows == [dict(base=0, ascii=False, leads=3, out=0, a=0)]
    m = D.Layout(b"\xd0\xb6" + b"x" * (D.ROW - 2) + b"y" * D.ROW + b"z" * 5)
    assert [(r["ascii"], r["leads"], r["out"], r["a"]) for r in m.rows] == \
        [(False, D.ROW - 1, 0, 0), (True, D.ROW, D.ROW - 1, 3), (False, 5, 2 * D.ROW - 1, 3)] and not m.dropped
    m = D.Layout(b"x" * D.ROW)   # a last row that is full is an ASCII row; one byte short, it is not
    assert m.rows[0]["ascii"] and not D.Layout(b"x" * (D.ROW - 1)).rows[0]["ascii"]
    assert D.Layout(b"\x80" * D.TILE + b"ab").tile_leads(0) == 0


def _is_cont(b):
    return b & 0xC0 == 0x80


def check_claims(name, text, vocab, expect, m):
    claims = dict(expect["claims"])
    assert claims, "every case states what it is"
    if "nbytes" in claims:
        assert len(text) == claims.pop("nbytes")
    if "n_text" in claims:
        assert m.n_text == claims.pop("n_text"), m.n_text
    assert m.dropped == claims.pop("dropped", m.dropped)
    for c in claims.pop("has", ()):
        assert c in m.text_used, hex(c)
    for c in claims.pop("lacks", ()):
        assert c not in m.text_used, hex(c)
    for c in claims.pop("vocab_only", ()):
        assert c in m.used and c not in m.text_used, hex(c)
    assert (m.alphabet > 255) == claims.pop("wide", False), m.alphabet
    if claims.pop("vocab_in_s", 0):
        assert m.text_used & {0, 1}
    else:
        assert not m.text_used & {0, 1}
    if "ends_with" in claims:
        assert text.endswith(claims.pop("ends_with"))
    if "boundary" in claims:
        kind, X = claims.pop("boundary")
        pos, s = claims.pop("lead")
        assert D.boundary_kind(X) == kind and pos == X - s and text[pos] >= 0x80 and text[pos - 1] < 0x80
        if claims.pop("rejected", False):
            assert pos not in m.starts and (X in m.starts) == _is_cont(text[pos]) and _is_cont(text[X]) == (text[pos] >= 0xC0)
        elif m.dropped:   # the last continuation byte is missing: the lead and what it has are dropped
            L = OM.seq_len(text[pos])
            assert pos not in m.starts and pos + L - 1 in m.starts and all(_is_cont(b) for b in text[pos + 1:pos + L - 1])
        else:             # a valid sequence with s bytes in front of the boundary and the rest behind it
            assert pos in m.starts and pos < X < pos + OM.seq_len(text[pos])
    for r, (ascii_row, a) in claims.pop("rows", {}).items():
        assert (m.rows[r]["ascii"], m.rows[r]["a"]) == (ascii_row, a), (r, m.rows[r])
    zero = claims.pop("zero_rows", ())
    for r in zero:
        assert m.rows[r]["leads"] == 0 and m.rows[zero[0] - 1]["leads"] > 0 and m.rows[zero[-1] + 1]["leads"] > 0
    for t in claims.pop("zero_tiles", ()):
        assert m.tile_leads(t) == 0 and m.tile_leads(t - 1) > 0 and m.tile_leads(t + 1) > 0
    assert not claims, claims


_ref = None


def _reference_decoder():
    """the reference's own decoder through the shim (oracle/_ref/librefutils.so), where it was built"""
    global _ref
    if _ref is None and os.path.exists(O.REFUTILS):
        _ref = C.CDLL(O.REFUTILS)
        _ref.ref_decode_utf8.restype = C.c_size_t
        _ref.ref_decode_utf8.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32)]
    return _ref


def check_references(text, vocab, m, fast):
    cps, invalid = O.decode_utf8(text)
    assert cps.tolist() == m.cps and invalid == m.dropped
    assert bruteforce.decode(text) == m.cps
    R = _reference_decoder()
    if R is not None:
        buf = (C.c_uint32 * (len(text) + 1))()
        assert list(buf[:R.ref_decode_utf8(text, len(text), buf)]) == m.cps
    ov = O.Vocab(vocab)
    ids, spans, t, starts = OM.encode_spans(text, vocab)
    assert ids == ov.encode(text).tolist() and (t, starts) == (m.cps, m.starts)
    OM.check_coverage(text, ids, spans, t, starts)
    if fast:
        assert ov.fast_encode(text).tolist() == fast_model(text, vocab)


@pytest.mark.parametrize("name", D.names("BAUM"))
def test_case_is_what_its_builder_claims(name):
    text, vocab, expect = D.build(name)
    m = D.Layout(text, vocab)
    check_claims(name, text, vocab, expect, m)
    check_references(text, vocab, m, expect["fast"])


E_BLOCKS = 24


@pytest.mark.parametrize("block", range(E_BLOCKS))
def test_end_case_is_what_its_builder_claims(block):
    for name in D.names("E")[block::E_BLOCKS]:
        text, vocab, expect = D.build(name)
        m = D.Layout(text, vocab)
        check_claims(name, text, vocab, expect, m)
        check_references(text, vocab, m, expect["fast"])


def test_dirty_tail_cases():
    """P: the text is an E text that ends in ASCII or in a cut-off lead; the 64 bytes behind it would complete the lead or
    add a line end"""
    for name in D.names("P"):
        text, vocab, expect = D.build(name)
        e_text = D.build("E_" + name[2:name.rindex("_")])[0]
        tail = expect["tail"]
        assert text == e_text and len(tail) == 64 and len(text) == expect["claims"]["nbytes"], name
        m, dirty = D.Layout(text), D.Layout(text + tail)
        if "_cut" in name:
            # (F0 80 80 80 is an overlong form: behind the lone lead, the 0x80 tail only adds bytes to drop)
            completes = 0 if name.endswith("cut3_80") else 1
            assert m.dropped and dirty.n_text == m.n_text + completes and dirty.cps[:m.n_text] == m.cps, name
        elif tail[0] == 0x0A:
            assert not m.dropped and (text + tail).count(b"\n") == text.count(b"\n") + 64, name
        else:
            assert not m.dropped and dirty.dropped, name


@pytest.mark.parametrize("name", D.names("H"))
def test_reuse_pair(name):
    second, vocab, expect = D.build(name)
    first, q = expect["first"], len(second)
    m = D.Layout(second, vocab)
    check_claims(name, second, vocab, expect, m)
    assert len(first) > q + 3 and all(_is_cont(b) for b in first[q:q + 3]), "the first text has continuation bytes at q, q + 1, q + 2"
    lead = m.starts[-1] + 1 if m.starts else 0   # the second text ends in a lead that its end cuts off
    assert second[lead] >= 0xC0 and q - lead < OM.seq_len(second[lead]) and all(_is_cont(b) for b in second[lead + 1:])
    missing = OM.seq_len(second[lead]) - (q - lead)
    completed = D.Layout(second + first[q:q + missing])   # what a reader of the first text's stale bytes would see
    assert completed.n_text == m.n_text + 1 and not completed.dropped
    if "conts_first" not in name:
        assert not D.Layout(first).dropped and first[:q] == second, "valid multi-byte text whose sequences line up that way"
    check_references(second, vocab, m, expect["fast"])
    check_references(first, vocab, D.Layout(first, vocab), expect["fast"])
