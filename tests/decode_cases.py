"""Inputs placed on the seams of the UTF-8 decode stage (csrc/decode.h, and the row loads that csrc/offsets.h and
csrc/normalize.h repeat), shared by test_decode_cases.py (no GPU) and test_gpu_decode_edges.py: the layout constants, read
from the headers by name; a plain-Python layout model over offsets_model.decode_with_starts that says, per 1 KB row, whether
the decoder takes the pure-ASCII flush, how many valid leads the row has and at which output position (and so at which
alignment a = out & 3) it is written, and for the text its code points, their first bytes, the used set and whether a byte
is dropped; and the cases, in groups

  B  a sequence that straddles a word / lane / row / wave / tile boundary (valid, cut short, rejected or accepted on the
     strength of a second byte that sits across the boundary), and C0 / C1 / F5 / a lone continuation byte in front of one;
  E  ends: every small length, the lengths around a chunk, row, wave and tile end, each ending in ASCII, in a complete
     sequence or in a lead that the end cuts off; invalid bytes only; whole rows and a whole tile without a lead; U+0000
     and U+0001 against the zero fill;
  A  the aligned flush of pure-ASCII rows at every output alignment, next to rows of the same wave, the next wave, the
     next tile, mixed rows and the ragged end;
  U  the same with more than 255 distinct code points (4-byte symbols), and the wave / tile straddles again;
  M  the three marking paths of the alphabet and the edges of a bitmap word;
  P  E texts with 64 "dirty" bytes behind nbytes in the device buffer (for the _device entry points);
  H  pairs of texts for one handle: the second ends in a lead cut off where the first has continuation bytes.

build(name) -> (text bytes, vocabulary lines, expect).  expect["claims"] is what the builder says it built (test_decode_cases.py
holds the layout model to it), expect["fast"] whether the fast entry point is compared, expect["soft"] whether the vocabulary
makes spacing chars soft.  P: expect["tail"] are the bytes behind the text; H: expect["first"] is the text encoded first.
Importing this module loads no library."""
import bisect
import os
import random
import re

import offsets_model as OM
from bruteforce import is_spacing

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "wordpiece_amd", "csrc")


def _constant(header, name):
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(r"^constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, f.read(), re.M)
    assert m, (header, name)
    return int(m.group(1))


# ---- the constants the cases stand on: a changed constant moves the cases with it
DEC_CHUNK = _constant("decode.h", "kDecChunk")   # bytes per lane and row
DEC_ROWS = _constant("decode.h", "kDecRows")     # rows per wave
LANES = _constant("common.h", "kWave")
BLOCK = _constant("common.h", "kBlock")
WORD = 4                                         # the SWAR word
CHUNK = DEC_CHUNK
ROW = LANES * CHUNK                              # decode.h, kDecRowBytes
WAVE = ROW * DEC_ROWS                            # decode.h, kDecWaveBytes
TILE = (BLOCK // LANES) * WAVE                   # decode.h, kDecTile
MAX_TEXT = 3 * TILE + ROW                        # no text is longer than three tiles and a ragged tail


# ---- the layout model -------------------------------------------------------------------------------------------------------

def vocab_code_points(vocab):
    """the vocabulary's share of the alphabet: the code points of every line's word (without "##"), vocab.h"""
    toks, _ = OM._vocab(vocab)
    return {c for _, _, cps in toks for c in cps}


def soft_set(vocab):
    """spacing chars that occur inside an eligible token of more than one symbol (vocab.h; walk_cases.Model.soft)"""
    toks, _ = OM._vocab(vocab)
    return {c for _, bad, w in toks if not bad and len(w) > 1 for c in w if is_spacing(c)}


class Layout:
    """What the two decode passes make of `text`: cps / starts (offsets_model.decode_with_starts), dropped (some byte is
    consumed by no code point), used (text, vocabulary and the separator 1: round0_cases.code_lengths), and per row r that
    holds a byte of the text rows[r] = dict(ascii=the row_ascii rule: every lane's chunk is pure ASCII and inside the
    text, leads=valid leads, out=output position of the row's first lead, a=out & 3)."""

    def __init__(self, text, vocab=()):
        self.nbytes = len(text)
        self.cps, self.starts = OM.decode_with_starts(text)
        self.n_text = len(self.cps)
        self.dropped = sum(OM.seq_len(text[s]) for s in self.starts) != len(text)
        self.text_used = set(self.cps)
        self.used = self.text_used | {1} | vocab_code_points(vocab)
        self.alphabet = len(self.used)
        self.rows = []
        for base in range(0, len(text), ROW):
            lo, hi = bisect.bisect_left(self.starts, base), bisect.bisect_left(self.starts, base + ROW)
            full = base + ROW <= len(text) and max(text[base:base + ROW]) < 0x80
            self.rows.append(dict(base=base, ascii=full, leads=hi - lo, out=lo, a=lo & 3))

    def tile_leads(self, t):
        return sum(r["leads"] for r in self.rows[t * (TILE // ROW):(t + 1) * (TILE // ROW)])

    def symbols(self):
        """dense symbol of every text position: rank of the code point in the used set, plus 1"""
        order = sorted(self.used)
        rank = {c: i + 1 for i, c in enumerate(order)}
        return [rank[c] for c in self.cps]


# ---- vocabularies -----------------------------------------------------------------------------------------------------------
C2, C3, C4 = "ж".encode(), "中".encode(), "😀".encode()   # D0 B6 / E4 B8 AD / F0 9F 98 80: no two continuation bytes alike
assert (C2, C3, C4) == (b"\xd0\xb6", b"\xe4\xb8\xad", b"\xf0\x9f\x98\x80")
BASE = ["[UNK]", "a", "b", "##a", "##b", "ab", "##ab", "ba", ",", ".", "-", "é", "##é", "ж", "##ж", "中", "😀", "##😀"]
SOFT = BASE + ["a,b", "a b", "中中"]                       # ',' ' ' and U+4E2D are soft
WIDE = BASE + [chr(c) for c in range(0x400, 0x400 + 300) if chr(c) != "ж"]   # more than 255 code points: 4-byte symbols
assert len(vocab_code_points(WIDE)) > 255 and soft_set(SOFT) == {44, 32, 0x4E2D} and not soft_set(BASE)

FILL = b"ab ,.-\t\n"   # class-dense: a class byte or symbol written one position off lands on a neighbour that differs


def fill(n, seed):
    return bytes(random.Random(seed).choices(FILL, k=n))


def patched(n, patches, seed):
    """n bytes of filler with `patches` ((position, bytes), ...) written over it"""
    b = bytearray(fill(n, seed))
    prev = 0
    for pos, p in sorted(patches):
        assert prev <= pos and pos + len(p) <= n, (prev, pos, len(p), n)
        b[pos:pos + len(p)] = p
        prev = pos + len(p)
    return bytes(b)


CASES = {}   # name -> (text or its maker, vocabulary, expect)


def later(f, *args, **kw):
    """the text is made when the case is asked for"""
    return lambda: f(*args, **kw)


def _add(name, text, vocab=BASE, fast=True, soft=False, **extra):
    """text (and first=): bytes, or a function without arguments that makes them (see later)"""
    assert name not in CASES, name
    claims = extra.pop("claims", {})
    CASES[name] = (text, vocab, dict(claims=claims, fast=fast, soft=soft, **extra))


# ---- B: straddles -----------------------------------------------------------------------------------------------------------
BOUNDARIES = {"word": 5 * ROW + 7 * CHUNK + 2 * WORD,   # a word boundary inside a lane's chunk
              "chunk": 5 * ROW + 7 * CHUNK,             # a lane boundary inside a row: w[r][4] by __shfl_down
              "row": WAVE + 2 * ROW,                    # lane 63 -> lane 0 of the wave's next row
              "wave": 2 * WAVE,                         # the broadcast `tail` load behind the wave
              "tile": TILE}                             # the same load, into the next workgroup's tile


def boundary_kind(x):
    return "tile" if x % TILE == 0 else "wave" if x % WAVE == 0 else "row" if x % ROW == 0 else \
        "chunk" if x % CHUNK == 0 else "word" if x % WORD == 0 else None


B_LEN = TILE + 37
VALID = {2: C2, 3: C3, 4: C4}
REJECTED = {"E09F": b"\xe0\x9f\xad", "EDA0": b"\xed\xa0\xad", "F08F": b"\xf0\x8f\x98\xad", "F490": b"\xf4\x90\x98\xad"}
ACCEPTED = {"E0A080": (b"\xe0\xa0\x80", 0x800), "ED9FBF": (b"\xed\x9f\xbf", 0xD7FF),
            "F0908080": (b"\xf0\x90\x80\x80", 0x10000), "F48FBFBF": (b"\xf4\x8f\xbf\xbf", 0x10FFFF)}
LAST_BYTE = {"C0": b"\xc0\xa9", "C1": b"\xc1\xa9", "F5": b"\xf5\x9f\x98\x80", "cont": b"\x80"}   # the first byte sits at X - 1


def _b_cases(prefix, vocab, kinds, valid_only=False):
    for k, kind in enumerate(kinds):
        X = BOUNDARIES[kind]
        for L in (2, 3, 4):
            for s in range(1, L):
                pos, seed = X - s, 100 * k + 10 * L + s
                at = dict(boundary=(kind, X), lead=(pos, s), wide=vocab is WIDE)
                _add("%s_%s_L%ds%d_valid" % (prefix, kind, L, s), later(patched, B_LEN, [(pos, VALID[L])], seed), vocab,
                     claims=dict(at, dropped=False, n_text=B_LEN - (L - 1), has=[ord(VALID[L].decode())]))
                if valid_only:
                    continue
                _add("%s_%s_L%ds%d_missing" % (prefix, kind, L, s), later(patched, B_LEN, [(pos, VALID[L][:-1] + b"a")], seed), vocab,
                     claims=dict(at, dropped=True, n_text=B_LEN - (L - 1), lacks=[ord(VALID[L].decode())]))
                for form, (seq, cp) in ACCEPTED.items():
                    if len(seq) == L:
                        _add("%s_%s_L%ds%d_acc_%s" % (prefix, kind, L, s, form), later(patched, B_LEN, [(pos, seq)], seed), vocab,
                             claims=dict(at, dropped=False, n_text=B_LEN - (L - 1), has=[cp]))
        if valid_only:
            continue
        for form, seq in REJECTED.items():   # the deciding second byte lies across the boundary from the lead
            _add("%s_%s_rej_%s" % (prefix, kind, form), later(patched, B_LEN, [(X - 1, seq)], 200 + k), vocab,
                 claims=dict(boundary=(kind, X), lead=(X - 1, 1), dropped=True, n_text=B_LEN - len(seq), rejected=True))
        for form, seq in LAST_BYTE.items():
            _add("%s_%s_last_%s" % (prefix, kind, form), later(patched, B_LEN, [(X - 1, seq)], 300 + k), vocab,
                 claims=dict(boundary=(kind, X), lead=(X - 1, 1), dropped=True, n_text=B_LEN - len(seq), rejected=True))


_b_cases("B", BASE, list(BOUNDARIES))

# ---- E: ends ----------------------------------------------------------------------------------------------------------------
E_KINDS = {"ascii": b"", "c2": C2, "c3": C3, "c4": C4, "cut1": C4[:3], "cut2": C4[:2], "cut3": C4[:1]}   # cutK: K bytes missing
E_AROUND = (CHUNK, ROW, WAVE, 2 * WAVE, TILE, 2 * TILE)
E_LENGTHS = sorted(set(range(1, 41)) | {x + d for x in E_AROUND for d in range(-5, 6)})


def _e_text(n, kind):
    tail = E_KINDS[kind]
    return fill(n - len(tail), 7000 + n) + tail


for _n in E_LENGTHS:
    for _kind, _tail in E_KINDS.items():
        if len(_tail) > _n:
            continue
        _cut = _kind.startswith("cut")
        _add("E_len%d_%s" % (_n, _kind), later(_e_text, _n, _kind),
             claims=dict(nbytes=_n, dropped=_cut, n_text=_n - len(_tail) + (1 if _kind[0] == "c" and not _cut else 0),
                         ends_with=_tail))
_add("E_invalid_only", b"\x80\xbf\xc0\xf5\xe4\xb8\xf0\x9f\x98\xff" * 11, claims=dict(dropped=True, n_text=0))
_add("E_invalid_only_tile", b"\x80\xbf\xc0\xf5\xe4\xb8\xf0\x9f\x98\xff" * ((TILE + 50) // 10), claims=dict(dropped=True, n_text=0))
_add("E_cont_rows", patched(TILE + 100, [(2 * ROW, b"\x80\xbf" * ROW)], 41),
     claims=dict(dropped=True, n_text=TILE + 100 - 2 * ROW, zero_rows=[2, 3]))
_add("E_cont_rows_across_waves", patched(TILE + 100, [(3 * ROW, b"\xbf\x80" * ROW)], 42),
     claims=dict(dropped=True, n_text=TILE + 100 - 2 * ROW, zero_rows=[3, 4]))
_add("E_cont_tile", patched(2 * TILE + 333, [(TILE, b"\x80\xbf" * (TILE // 2))], 43),
     claims=dict(dropped=True, n_text=TILE + 333, zero_tiles=[1]))
_add("E_cont_wave", patched(TILE + 100, [(WAVE, b"\x80" * WAVE)], 44),
     claims=dict(dropped=True, n_text=TILE + 100 - WAVE, zero_rows=[4, 5, 6, 7]))
for _c in (0, 1):   # U+0000 / U+0001 are code points of the text, not the zero fill behind it (and 1 is the separator of S)
    _add("E_u%04x_last_of_row" % _c, patched(2 * ROW + 10, [(ROW - 1, bytes([_c]))], 50 + _c),
         claims=dict(dropped=False, n_text=2 * ROW + 10, has=[_c], vocab_in_s=1, rows={0: (True, 0)}))
    _add("E_u%04x_last_of_text" % _c, fill(ROW + 21, 52 + _c) + bytes([_c]),
         claims=dict(dropped=False, n_text=ROW + 22, has=[_c], vocab_in_s=1))
    _add("E_u%04x_last_of_text_full_row" % _c, fill(ROW - 1, 54 + _c) + bytes([_c]),
         claims=dict(dropped=False, n_text=ROW, has=[_c], vocab_in_s=1, rows={0: (True, 0)}))


# ---- A: alignment of the ASCII flush ------------------------------------------------------------------------------------------
# row 0 holds j two-byte characters, so row 1 is written at out = ROW - j: a = (-j) & 3.  Rows (A pure ASCII, M mixed with
# four two-byte characters, which keeps a): 0 M, 1-4 A (2 follows 1 in its wave, 4 follows 3 across the wave boundary), 5 M
# (behind an A row), 6 A (behind a mixed row), 7-17 A (16 follows 15 across the tile boundary), 18 the ragged end
A_ROWS = 18
A_MIXED = 5


def _a_text(j, seed, ragged=37, extra=()):
    two = [C2, "é".encode(), "Ж".encode(), "я".encode()]
    row0 = [(8 + 40 * i, two[i % 4]) for i in range(j)]
    mixed = [(A_MIXED * ROW + 100 * i + 3, two[i]) for i in range(4)]
    return patched(A_ROWS * ROW + ragged, row0 + mixed + list(extra), seed)


def _a_claims(a, ragged=37):
    rows = {r: (True, a) for r in list(range(1, A_MIXED)) + list(range(A_MIXED + 1, A_ROWS))}
    rows[0] = (False, 0)
    rows[A_MIXED] = (False, a)
    rows[A_ROWS] = (False, a)   # the ragged end: never the aligned flush
    return dict(dropped=False, rows=rows, nbytes=A_ROWS * ROW + ragged)


for _j in (4, 1, 2, 3):
    _a = (-_j) & 3
    _add("A_a%d" % _a, later(_a_text, _j, 600 + _j), claims=_a_claims(_a))
    _add("A_a%d_soft" % _a, later(_a_text, _j, 600 + _j), SOFT, fast=False, soft=True, claims=_a_claims(_a))
    # the ragged end nearly a row: only its last lane's chunk is cut
    _add("A_a%d_long_end" % _a, later(_a_text, _j, 610 + _j, ragged=ROW - 3), claims=_a_claims(_a, ROW - 3))

# ---- U: 4-byte symbols --------------------------------------------------------------------------------------------------------
for _j in (4, 1, 2, 3):
    _a = (-_j) & 3
    _add("U_a%d" % _a, later(_a_text, _j, 700 + _j), WIDE, claims=dict(_a_claims(_a), wide=True))
    # astral characters among them: rows 3 and 17 become mixed rows, the rows behind them move to other alignments
    _add("U_a%d_astral" % _a, later(_a_text, _j, 700 + _j, extra=[(3 * ROW + 17, C4 + C3), (A_ROWS * ROW - 40, C4)]), WIDE,
         claims=dict(dropped=False, wide=True, has=[0x1F600, 0x4E2D], nbytes=A_ROWS * ROW + 37,
                     rows={1: (True, _a), 2: (True, _a), 3: (False, _a), 4: (True, (_a - 5) & 3), 17: (False, (_a - 9) & 3)}))
_b_cases("U", WIDE, ["wave", "tile"], valid_only=True)

# ---- M: alphabet marking ------------------------------------------------------------------------------------------------------
M_EDGES = [0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000, 0x10FFFF, 0x3FF, 0x400, 0x41F, 0x420, 0xFFE0, 0xFFDF, 0x1001F, 0x10020]
_edges = "".join(chr(c) for c in M_EDGES).encode()
_add("M_edges_small", fill(200, 80) + _edges + fill(77, 81), claims=dict(dropped=False, has=M_EDGES))
_add("M_edges_tile_end", later(patched, TILE + 500, [(TILE - len(_edges) + 11, _edges)], 82), claims=dict(dropped=False, has=M_EDGES))
_add("M_edges_wide", fill(200, 83) + _edges + fill(77, 84), WIDE, claims=dict(dropped=False, has=M_EDGES, wide=True))
_add("M_edges_soft", fill(200, 85) + _edges + fill(77, 86), SOFT, fast=False, soft=True, claims=dict(dropped=False, has=M_EDGES))
_rare = "☃".encode()
_add("M_same_rare_two_tiles", patched(TILE + 900, [(1234, _rare), (TILE + 321, _rare), (TILE + 600, C4), (77, C4)], 87),
     claims=dict(dropped=False, has=[0x2603, 0x1F600], n_text=TILE + 900 - 2 * 2 - 2 * 3))
_add("M_vocab_only", fill(3000, 88), BASE + ["Ω", "##𝄞"], claims=dict(dropped=False, vocab_only=[0x3A9, 0x1D11E], n_text=3000))
_add("M_ascii_flags", bytes(range(0, 128)) * 9, claims=dict(dropped=False, has=list(range(128)), vocab_in_s=1, rows={0: (True, 0)}))

# ---- P: dirty tails behind nbytes ---------------------------------------------------------------------------------------------
P_TAILS = {"BF": b"\xbf" * 64, "80": b"\x80" * 64, "0A": b"\x0a" * 64}
for _n in E_LENGTHS:
    for _kind in ("ascii", "cut1", "cut2", "cut3"):
        if len(E_KINDS[_kind]) > _n:
            continue
        for _tn in (("0A", "BF") if _kind == "ascii" else ("BF", "80")):
            _add("P_len%d_%s_%s" % (_n, _kind, _tn), later(_e_text, _n, _kind), tail=P_TAILS[_tn], claims=dict(nbytes=_n))

# ---- H: reuse of a handle's staging ---------------------------------------------------------------------------------------------
H_Q = (5, CHUNK, CHUNK + 1, 2 * CHUNK - 1, ROW, ROW + 1, WAVE - 1, WAVE, TILE, TILE + 3)
for _q in H_Q:
    _head = fill(_q - 1, 900 + _q)
    # the first is valid text whose astral character has its continuation bytes at q, q + 1, q + 2; the second ends in its lead
    _add("H_q%d_valid_first" % _q, _head + C4[:1], first=_head + C4 + fill(30, 901), claims=dict(nbytes=_q, dropped=True, n_text=_q - 1))
    _add("H_q%d_cut2_conts_first" % _q, fill(_q - 2, 905 + _q) + C4[:2], first=fill(_q, 905 + _q) + b"\x98\x80\xbf" + fill(30, 902),
         claims=dict(nbytes=_q, dropped=True, n_text=_q - 2))
    _add("H_q%d_conts_first" % _q, fill(_q - 3, 903 + _q) + C4[:3], first=fill(_q, 903 + _q) + b"\xbf\xbf\xbf" + fill(30, 904),
         claims=dict(nbytes=_q, dropped=True, n_text=_q - 3))

GROUPS = ("B", "E", "A", "U", "M", "P", "H")
GROUP_SIZES = {"B": 150, "E": 668, "A": 12, "U": 20, "M": 7, "P": 754, "H": 30}   # asserted by test_decode_cases.py


def names(groups="BEAUM"):
    return [n for n in CASES if n[0] in groups]


def build(name):
    """-> (text bytes, vocab lines, expect)"""
    text, vocab, expect = CASES[name]
    expect = dict(expect)
    if callable(text):
        text = text()
    if callable(expect.get("first")):
        expect["first"] = expect["first"]()
    assert len(text) <= MAX_TEXT, (name, len(text))
    return text, vocab, expect
