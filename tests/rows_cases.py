"""Constructed inputs for the documents layer — csrc/rows.h (line_ends16, line_count_kernel, line_write_kernel, cp_at_byte,
row_splits_kernel, row_of_id, rebase_kernel, pack_rows_kernel), what a normalised handle adds in csrc/normalize.h
(norm_doc_starts_kernel, norm_fill_starts_kernel, norm_row_base_kernel) and LinearPath::row_structure — with what every case
claims.  Shared by test_rows_cases.py (CPU) and test_gpu_rows_edges.py.  Importing this module loads no library.

build(name) -> Case, which unpacks as (docs or text, vocab, mode, claims).  mode "docs": a list of documents (explicit rows,
lines, and lines with the open end); mode "lines": a text as it stands, open-ended or not (one that ends in '\n' is also run
with the explicit starts of its lines and without its last byte).  Expected results come only from rows_model (row i = the
per-document encode) and, for a normalised handle, normalize_model.encode_spans_normalized per document: expected().

C = kDecChunk = 16 bytes per lane, I = kBlock * C = 4096 bytes per iteration, T = kLineTile = kLineIters * I = 16 KB per
workgroup of the line kernels, RT = kRebaseTile = kBlock * kRebaseItems = 2048 ids per workgroup of the rebase.

edge (issue bullet)                                            case(s)
L  '\n' at each of the 16 bytes of a chunk                     L_nl_each_byte
   '\n' at 1023 | 1024, at T - 1 | T                           L_nl_1023 L_nl_1024 L_nl_1023_1024 L_nl_T-1 L_nl_T L_nl_T-1_T
   '\n' at both edges of the four iterations of a tile         L_nl_iter_edges_tile0, L_nl_iter_edges_tile1
   lengths 1 15 16 17 32 T-1 T T+1 2T, '\n' at the end / open  L_len_<n>_nl, L_len_<n>_open (last byte a word), L_len_32_open_blank
   16 newlines filling a chunk; 300 across a tile edge         L_chunk_of_16, L_run_300
   newlines only, below and above a tile (no ids: memset)      L_only_nl_100, L_only_nl_T+77
   0x8A on a chunk's / a tile's last byte, '\n' on both sides: L_8a_cp2_chunk L_8a_cp2_tile (U+010A), L_8a_cp3_chunk L_8a_cp3_tile
   second byte, third byte, lone; and as the open end          (U+4E8A), L_8a_lone_chunk L_8a_lone_tile, L_8a_open_end
   E4 B8 0A; lines of invalid bytes only                       L_trunc_before_nl, L_invalid_lines
S  a start behind 5 100 5000 code points of 2 3 4 bytes        S_behind_<k>_<w>   (k = 5000, w = 3 4: the start byte is above n_text)
   a probe of the gallop lands on the answer itself (step 2^j) S_probe_hit_<k> (k = 2^(j+1) - 1 two-byte code points in front),
   from the start byte / from the clamp n_text                 S_probe_hit_clamped
   a last boundary / a last document behind trailing blanks,   S_trailing_blanks S_trailing_invalid S_last_doc_blanks
   trailing invalid bytes                                      S_last_doc_invalid
   empty / blank / invalid documents first, last, in a row,    S_first_<kind> S_last_<kind> (kind: empty blank invalid), S_consecutive,
   as the whole batch                                          S_all_<kind>_1, S_all_<kind>_3
   255 256 257 rows                                            S_rows_<n>
   a failing word first in its document                        S_unk_first
B  a row boundary at id 2047 2048 2049 4095 4096               B_bound_<k>
   one row over ids 100..5000 (tile 1 inside one row)          B_row_100_5000
   2048 / 2049 rows of one id; n_ids 2048 / 2049               B_rows_2048 B_rows_2049, B_nids_2048 B_nids_2049
   300 empty rows in front of id 2048                          B_empty_300
   (every B case starts with 2-, 3- and 4-byte words: the byte base and the code-point base of every later row differ)
P  max_len x specials x n_rows x row lengths                   pack_batches(max_len): P_<max_len>
N  documents that begin / end with dropped code points         N_begin_dropped_f<F>, N_end_dropped_f<F>   (F = 1 4 7)
   dropped only: in the middle, last (the open end: a last     N_only_dropped_middle_f<F>, N_only_dropped_last_f<F>,
   line that normalises to nothing), every document            N_only_dropped_all_1_f<F> (open end: a text that normalises to
                                                               nothing), N_only_dropped_all_3_f<F>
   documents that begin with an expanding code point           N_begin_expands_f<F>
   a document in front that grows / shrinks by > C bytes       N_front_grows_f<F>, N_front_shrinks_f<F>
   fewer / more source line tiles than normalised ones         N_tiles_hangul_f<F> (1 -> 2 for F = 4 7), N_tiles_zwsp_f<F> (2 -> 1 for 1 7)
C  L, S, B together at three tiles; N with them at three       C_plain, C_norm_f7

What drops under a flag set: Cf and U+0000 under WP_NORM_CLEAN, Mn under WP_NORM_STRIP_ACCENTS; DROP[F] holds only code points
that F drops.  Under F = 4 the issue's U+200B / U+0000 / U+FEFF stay in the text (unknown words), under F = 1 the marks do.

Wall time (measured on the build container, single-threaded): test_rows_cases.py 9 s for its 143 tests (the whole CPU suite
with it: 384 s for 1163 tests); test_gpu_rows_edges.py: 7.5 s for its 142 tests on an MI355X (the figures and the mutation
counts stand in that file's docstring)."""
import functools
import os
import re

import normalize_model as NM
import offsets_model as OM
import rows_model as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wordpiece_amd", "csrc")


def _constant(header, name):
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(r"^constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, f.read(), re.M)
    assert m, (header, name)
    return int(m.group(1))


# ---- the constants the cases stand on: a changed constant moves the cases with it
CHUNK = _constant("decode.h", "kDecChunk")
LINE_ITERS = _constant("rows.h", "kLineIters")
REBASE_ITEMS = _constant("rows.h", "kRebaseItems")
BLOCK = _constant("common.h", "kBlock")
WAVE = _constant("common.h", "kWave")
ITER = BLOCK * CHUNK                  # bytes per iteration of a line workgroup
T = ITER * LINE_ITERS                 # rows.h, kLineTile
RT = BLOCK * REBASE_ITEMS             # rows.h, kRebaseTile
ROW = WAVE * CHUNK                    # decode.h, kDecRowBytes: the decoder's row edge
MAX_TEXT = 3 * T + 2048               # no text is longer than three tiles and a little
assert (CHUNK, LINE_ITERS, REBASE_ITEMS, BLOCK, WAVE) == (16, 4, 8, 256, 64) and T == 16384 and RT == 2048 and ROW == 1024

# single letters and ## letters; U+010A and U+4E8A (their last byte is 0x8A); one spacing char of 2, 3 and 4 bytes, each a word
# of its own wherever it stands.  A document of n blank-separated words of these has exactly n ids.
WIDE = ("·", "中", "\U00020000")
PLAIN = ["[UNK]", "a", "b", "c", "##a", "##b", "##c", "Ċ", "亊"] + list(WIDE)
# a normalised handle: what the flag sets make of U+00C9 (E / e / itself) and of U+AC01 (itself / three jamo)
NORM = ["[UNK]", "a", "b", "c", "##a", "##b", "##c", "e", "E", "É", "##e", "##E", "##É", "각", "ᄀ", "##ᅡ", "##ᆨ"]
FLAG_SETS = (1, 4, 7)
DROP = {1: "\u200b\x00\ufeff", 4: "\u0301\u0300", 7: "\u200b\x00\u0301\ufeff"}
CLS, SEP, PAD = 101, 102, 77          # (no id of a vocabulary here)


class Case:
    def __init__(self, name, data, vocab, mode, claims, flags=0):
        assert mode in ("docs", "lines")
        self.name, self.data, self.vocab, self.mode, self.claims, self.flags = name, data, list(vocab), mode, dict(claims), flags
        if mode == "docs":
            self.data = [d if isinstance(d, bytes) else d.encode("utf-8") for d in data]
            assert not any(b"\n" in d for d in self.data), name
            self.text, self.starts = R.join_docs(self.data)
        else:
            self.text, self.starts = bytes(data), None
        assert len(self.text) <= MAX_TEXT, (name, len(self.text))

    def __iter__(self):
        return iter((self.data, self.vocab, self.mode, self.claims))

    def runs(self):
        """[(label, text, explicit starts or None, rows)]: what the GPU file calls and the rows it expects"""
        rows = R.split_lines(self.text)
        out = [("lines", self.text, None, rows)]
        if self.text.endswith(b"\n"):
            starts = [0]
            for r in rows:
                starts.append(starts[-1] + len(r) + 1)
            assert self.mode == "lines" or (rows == self.data and starts == self.starts), self.name
            out.insert(0, ("explicit", self.text, starts, rows))
            out.append(("lines, open end", self.text[:-1], None, R.split_lines(self.text[:-1])))
        return out


@functools.lru_cache(maxsize=None)
def model(vocab):
    return R.Model(list(vocab))


_MEMO = {}


def encode_doc(vocab, flags, doc, unit):
    """(ids, offsets) of one document: rows_model for a plain handle, normalize_model for a normalised one"""
    key = (tuple(vocab), flags, unit, doc)
    got = _MEMO.get(key)
    if got is None:
        if flags:
            got = NM.encode_spans_normalized(doc, list(vocab), flags, unit)
        else:
            got = model(tuple(vocab)).encode_with_offsets(doc, unit)
        got = _MEMO[key] = (list(got[0]), [tuple(o) for o in got[1]])
    return got


def expected(case_, rows, unit):
    """the contract: (ids, row_splits, offsets or None), row i = the encode of rows[i] alone"""
    ids, splits, offs = [], [0], []
    for d in rows:
        i, o = encode_doc(case_.vocab, case_.flags, d, unit or "byte")
        ids += i
        offs += o
        splits.append(len(ids))
    return ids, splits, (offs if unit else None)


CASES = {}


def case(name):
    def deco(f):
        assert name not in CASES, name
        CASES[name] = f
        return f
    return deco


# ---- family L: line ends ------------------------------------------------------------------------------------------------------

def _fill(n):
    """n bytes "a b c a b c ...": a letter at every even byte, a blank at every odd one"""
    return bytearray((b"a b c " * (n // 6 + 1))[:n])


def _lines_case(name, n, newlines, end="nl", patch=None, extra=None):
    """a text of n bytes with '\n' at exactly `newlines` (and at n - 1 with end == "nl"; end == "open": the last byte is the
    word "b"); patch: {byte position: bytes} written over the filling"""
    @case(name)
    def _():
        t = _fill(n)
        nl = sorted(set(newlines) | ({n - 1} if end == "nl" else set()))
        assert all(0 <= p < n for p in nl) and (end == "nl" or n - 1 not in nl), name
        for p in nl:
            t[p] = 0x0A
        if end == "open":
            t[n - 1] = ord("b")
            if n >= 2 and n - 2 not in nl:
                t[n - 2] = 0x20
        for pos, bs in (patch or {}).items():
            t[pos:pos + len(bs)] = bs
        assert len(t) == n
        claims = dict(len=n, len_mod16=n % CHUNK, len_mod_tile=n % T, newlines=nl, open_end=end != "nl")
        claims.update(extra or {})
        return Case(name, bytes(t), PLAIN, "lines", claims)


_lines_case("L_nl_each_byte", 16 * CHUNK + 9, [CHUNK * k + k for k in range(16)], end="open",
            extra=dict(newline_bytes_of_chunk=list(range(16))))
_lines_case("L_nl_1023", ROW + 77, [ROW - 1])
_lines_case("L_nl_1024", ROW + 77, [ROW])
_lines_case("L_nl_1023_1024", ROW + 77, [ROW - 1, ROW], extra=dict(empty_rows=1))
_lines_case("L_nl_T-1", T + 77, [T - 1])
_lines_case("L_nl_T", T + 77, [T], end="open")
_lines_case("L_nl_T-1_T", T + 77, [T - 1, T], extra=dict(empty_rows=1))
_lines_case("L_nl_iter_edges_tile0", T + 40, [0] + [j * ITER + d for j in range(1, LINE_ITERS + 1) for d in (-1, 0)], end="open")
_lines_case("L_nl_iter_edges_tile1", 2 * T + 40, [7, T - 9] + [T + j * ITER + d for j in range(0, LINE_ITERS + 1) for d in (-1, 0)])


def _inner(n):
    """a few line ends inside a text of n bytes: near the front, in the middle, every 1000 bytes"""
    return sorted({p for p in [5, n // 2] + list(range(999, n - 2, 1000)) if 0 < p < n - 2})


LENGTHS = ((1, "1"), (15, "15"), (16, "16"), (17, "17"), (32, "32"), (T - 1, "T-1"), (T, "T"), (T + 1, "T+1"), (2 * T, "2T"))
for _n, _nm in LENGTHS:
    _lines_case("L_len_%s_nl" % _nm, _n, _inner(_n))
    _lines_case("L_len_%s_open" % _nm, _n, _inner(_n), end="open")
_lines_case("L_len_32_open_blank", 32, [5], end="open", patch={30: b"c "})
_lines_case("L_chunk_of_16", 100, list(range(2 * CHUNK, 3 * CHUNK)), extra=dict(empty_rows=15))
_lines_case("L_run_300", T + 400, list(range(T - 150, T + 150)), extra=dict(empty_rows=299))


def _only_newlines(name, n):
    @case(name)
    def _():
        return Case(name, b"\n" * n, PLAIN, "lines", dict(len=n, len_mod16=n % CHUNK, len_mod_tile=n % T, newlines=list(range(n)),
                                                           open_end=False, n_ids=0, empty_rows=n))


_only_newlines("L_only_nl_100", 100)
_only_newlines("L_only_nl_T+77", T + 77)


def _8a_case(name, last, seq):
    """`seq` ends with 0x8A on byte `last` (a chunk's or a tile's last byte); '\n' right in front of it and right behind"""
    first = last - len(seq) + 1
    _lines_case(name, last + 30, [first - 1, last + 1], patch={first: seq}, extra=dict(byte_0x8a=[last]))


for _where, _last in (("chunk", 2 * CHUNK - 1), ("tile", T - 1)):
    _8a_case("L_8a_cp2_%s" % _where, _last, "Ċ".encode())
    _8a_case("L_8a_cp3_%s" % _where, _last, "亊".encode())
    _8a_case("L_8a_lone_%s" % _where, _last, b"\x8a")
# the open end is the 0x8A of U+010A, on bit 15 of the last chunk of a text of two whole chunks
_lines_case("L_8a_open_end", 2 * CHUNK, [12], end="open", patch={2 * CHUNK - 2: "Ċ".encode()}, extra=dict(byte_0x8a=[2 * CHUNK - 1]))
# E4 B8 0A: the lead and one continuation byte of a 3-byte sequence, cut short by the line end (bytes 13 14 | 15)
_lines_case("L_trunc_before_nl", 40, [15, 30], patch={13: b"\xe4\xb8"})


@case("L_invalid_lines")
def _():
    text = b"\xff\xfe\n\x80\x80\x80\n a\n\xc3\n\xe4\xb8\n\xf0\x9f\x98\nb \xff\n\x8a"
    nl = [i for i, b in enumerate(text) if b == 0x0A]
    return Case("L_invalid_lines", text, PLAIN, "lines", dict(len=len(text), len_mod16=len(text) % CHUNK, len_mod_tile=len(text) % T,
                                                             newlines=[2, 6, 9, 11, 14, 18, 22], open_end=True, n_ids=2, empty_rows=6,
                                                             n_rows=len(nl) + 1))


# ---- family S: starts to ids ------------------------------------------------------------------------------------------------------

def _docs_case(name, docs, claims=None, vocab=PLAIN, flags=0):
    @case(name)
    def _():
        d = docs() if callable(docs) else docs
        c = dict(n_rows=len(d))
        c.update(claims or {})
        return Case(name, d, vocab, "docs", c, flags)


def _behind(k, w):
    ch = WIDE[w - 2]
    assert len(ch.encode()) == w
    # the second document starts behind k code points of w bytes: at byte k * w + 1, code point k + 1
    _docs_case("S_behind_%d_%d" % (k, w), [ch * k, "a b", "c"],
               dict(splits_at=[k, k + 2], start_minus_cp=k * (w - 1), start_above_n_text=int(k * w + 1 > k + 1 + 4 + 2)))


for _k in (5, 100, 5000):
    for _w in (2, 3, 4):
        _behind(_k, _w)


def _probe_hit(k):
    # the start is byte b = 2 k + 1 <= n_text and code point p = k + 1; the gallop probes b - 1, b - 3, b - 7, ...: b - k = p
    _docs_case("S_probe_hit_%d" % k, ["·" * k, "a b", "a " * (k + 5)], dict(splits_at=[k, k + 2], probe_hit=1, start_above_n_text=0))


for _k in (1, 3, 7, 15, 31, 63):
    _probe_hit(_k)
# the start is byte 31 > n_text = 18: the gallop starts at the clamp and probes 17, 15, 11 = the answer
_docs_case("S_probe_hit_clamped", ["中" * 10, "a b", "c "], dict(splits_at=[10, 12], probe_hit=1, start_above_n_text=1))
_docs_case("S_trailing_blanks", ["a b", "c  \t "], dict(splits_at=[2, 3], empty_rows=0))
_docs_case("S_trailing_invalid", ["a b", b"c\xff\xfe\x80"], dict(splits_at=[2, 3], empty_rows=0))
_docs_case("S_last_doc_blanks", ["a b", " \t  "], dict(splits_at=[2], empty_rows=1, n_ids=2))
_docs_case("S_last_doc_invalid", ["a b", b"\xff\xfe\x80"], dict(splits_at=[2], empty_rows=1, n_ids=2))
KINDS = (("empty", b""), ("blank", b" \t  "), ("invalid", b"\xff\x80\xc3"))
for _kind, _d in KINDS:
    _docs_case("S_first_%s" % _kind, [_d, "a b", "c"], dict(splits_at=[0, 2], empty_rows=1))
    _docs_case("S_last_%s" % _kind, ["a b", "c", _d], dict(splits_at=[2, 3], empty_rows=1))
    _docs_case("S_all_%s_1" % _kind, [_d], dict(empty_rows=1, n_ids=0))
    _docs_case("S_all_%s_3" % _kind, [_d, _d + _d, _d], dict(empty_rows=3, n_ids=0))
_docs_case("S_consecutive", ["a", b"", b" ", b"\xff", b"", b"\x80 ", "b c", b"", b""], dict(splits_at=[1, 3], empty_rows=7, n_ids=3))
for _n in (BLOCK - 1, BLOCK, BLOCK + 1):   # one thread per boundary: n_rows + 1 of them
    _docs_case("S_rows_%d" % _n, ["b c" if i % 3 == 0 else "" if i % 7 == 3 else "a" for i in range(_n)], dict(n_rows=_n))
# "z" is in no token: the word fails, its span begins at the word's first code point — in its own document (the header's
# section "documents": "a failing first word belongs to its own document")
_docs_case("S_unk_first", ["a b", "zz a", "az b", "a z", "z", "c"], dict(splits_at=[2, 4, 6, 8, 9], n_ids=10, unk_first_rows=[1, 2, 4]))


# ---- family B: the rebase -----------------------------------------------------------------------------------------------------------

def _doc(count, wide=0):
    """a document of `count` one-symbol words: `wide` of them the 2-, 3- and 4-byte ones, in front"""
    wide = min(wide, count)
    return " ".join([WIDE[i % 3] for i in range(wide)] + ["abc"[i % 3] for i in range(count - wide)]).encode()


def _counts_case(name, counts, claims):
    """documents of counts[i] ids; the first one starts with three multi-byte words"""
    _docs_case(name, lambda: [_doc(c, 3 if i == 0 else 0) for i, c in enumerate(counts)],
               dict(claims, n_ids=sum(counts), empty_rows=sum(1 for c in counts if c == 0)))


for _k in (RT - 1, RT, RT + 1, 2 * RT - 1, 2 * RT):
    _counts_case("B_bound_%d" % _k, [3, _k - 3, 50], dict(splits_at=[3, _k]))
_counts_case("B_row_100_5000", [100, 4900, 60], dict(splits_at=[100, 5000], tile_inside_row=1))
_counts_case("B_rows_2048", [1] * RT, dict(splits_at=[1, RT - 1], n_rows=RT))
_counts_case("B_rows_2049", [1] * (RT + 1), dict(splits_at=[1, RT], n_rows=RT + 1))
_counts_case("B_empty_300", [RT] + [0] * 300 + [40], dict(splits_at=[RT], n_rows=302))
_counts_case("B_nids_2048", [700, 0, RT - 700], dict(splits_at=[700]))
_counts_case("B_nids_2049", [700, 0, RT + 1 - 700], dict(splits_at=[700]))


# ---- family P: the padded pack ------------------------------------------------------------------------------------------------------
MAX_LENS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 129, 200)


def lanes_for(max_len):
    """rows.h, lanes_for: lanes of a wave that share a row"""
    lanes = 4
    while lanes < WAVE and lanes < max_len:
        lanes *= 2
    return lanes


def pack_batches(max_len):
    """[(cls_id, sep_id, documents)]: the four combinations of specials that fit; 1, r - 1, r, r + 1 and 3 r + 2 rows, r the
    rows of a workgroup; row lengths 0, keep - 1, keep, keep + 1 and 3 max_len in turn (a single row: keep + 1)"""
    out = []
    r = BLOCK // lanes_for(max_len)
    for cls_id, sep_id in ((None, None), (CLS, None), (None, SEP), (CLS, SEP)):
        room = max_len - (cls_id is not None) - (sep_id is not None)
        if room < 0:
            continue
        lens = [0, max(0, room - 1), room, room + 1, 3 * max_len]
        for k, n_rows in enumerate((1, r - 1, r, r + 1, 3 * r + 2)):
            out.append((cls_id, sep_id, [_doc(lens[(i + k + 3) % 5]) for i in range(n_rows)]))
    return out


# ---- family N: a normalised handle ---------------------------------------------------------------------------------------------------
HANGUL = "각"     # an LVT syllable: three jamo (3 -> 9 bytes) under WP_NORM_STRIP_ACCENTS
E_ACUTE = "É"    # itself under 1, "E" under 4, "e" under 7 (2 -> 1 bytes)


def _n_case(name, docs_of, claims_of=None):
    for f in FLAG_SETS:
        _docs_case("%s_f%d" % (name, f), functools.partial(docs_of, f), claims_of(f) if claims_of else None, vocab=NORM, flags=f)


_n_case("N_begin_dropped", lambda f: ["a", "\u200ba b", "\x00c", "\ufeffa", DROP[f] + "b c", DROP[f][0] + " a", "b"])
_n_case("N_end_dropped", lambda f: ["a b\u200b", "c\ufeff", "a\x00", "b c" + DROP[f], "a " + DROP[f][-1], "b"])
_n_case("N_only_dropped_middle", lambda f: ["a", DROP[f], "b c", DROP[f][0], DROP[f] * 7, "a"], lambda f: dict(dropped_rows=[1, 3, 4]))
# (the header's section "documents": a line that the rule drops is still a row, also the last line of an open-ended text and
# the only line of a text that normalises to nothing — the open ends of the next two cases)
_n_case("N_only_dropped_last", lambda f: ["a b", "c", DROP[f]], lambda f: dict(dropped_rows=[2]))
_n_case("N_only_dropped_all_1", lambda f: [DROP[f]], lambda f: dict(dropped_rows=[0], n_ids=0))
_n_case("N_only_dropped_all_3", lambda f: [DROP[f], DROP[f][0], DROP[f] * 3], lambda f: dict(dropped_rows=[0, 1, 2], n_ids=0))
_n_case("N_begin_expands", lambda f: ["a", HANGUL + " a", E_ACUTE + " b", HANGUL, E_ACUTE, HANGUL + E_ACUTE + "a", "c"])
_n_case("N_front_grows", lambda f: [(HANGUL + " ") * 40, "a b", HANGUL + " c", "a"],
        lambda f: dict(front_delta=0 if f == 1 else 240))
_n_case("N_front_shrinks", lambda f: ["a\u200b\u0301 " * 40, "a b", E_ACUTE + " c", "a"],
        lambda f: dict(front_delta={1: -120, 4: -80, 7: -200}[f]))
# 2200 syllables in lines of five: 8.8 KB of source, 22 KB normalised under 4 and 7
_n_case("N_tiles_hangul", lambda f: [" ".join([HANGUL] * 5)] * 440,
        lambda f: dict(src_tiles=1, norm_tiles=1 if f == 1 else 2))
# 4000 words "a<U+200B>" in lines of eight: 20 KB of source, 8 KB normalised under 1 and 7
_n_case("N_tiles_zwsp", lambda f: [" ".join(["a\u200b"] * 8)] * 500,
        lambda f: dict(src_tiles=2, norm_tiles=2 if f == 4 else 1))


# ---- composed: the families in one batch of about three tiles --------------------------------------------------------------------------

@case("C_plain")
def _():
    docs = [WIDE[1] * 5000]                           # S: 5000 3-byte words in front; B: tiles 1 and the id 4096 inside row 0
    docs += [b""] * 300                               # B / S: 300 empty rows in front of id 5000
    docs += ["a Ċ 亊 b".encode() + b" \x8a \xe4\xb8"]   # L: 0x8A three ways, a truncated sequence in front of the '\n'
    at = sum(len(d if isinstance(d, bytes) else d.encode()) + 1 for d in docs)
    docs += [b" " * (T - 1 - at)]                     # L: a document of blanks whose '\n' is the first tile's last byte
    docs += ["a b c"]                                 # ... and a document that starts with the second tile
    docs += [_doc(3 * RT - (5000 + 4 + 3))]           # B: the next boundary is id 3 * RT
    docs += ["abc"[i % 3] for i in range(1200)]       # B: rows of one id
    docs += ["zz a", b"\xff\xfe", _doc(6000), "az", " \t "]   # S: failing first words, an invalid row, a last row of blanks
    return Case("C_plain", docs, PLAIN, "docs", dict(newline_at=[T - 1], splits_at=[5000, 3 * RT], n_rows=len(docs), min_tiles=3))


@case("C_norm_f7")
def _():
    f = 7
    docs = [(HANGUL + " ") * 1500]                    # N: 6 KB of source, 15 KB normalised: every later offset differs
    docs += [DROP[f]] + [""] * 100
    docs += ["a\u200b " * 3000]                       # N: 15 KB of source, 6 KB normalised
    docs += ["\u200b" + E_ACUTE + " a", HANGUL, "\ufeff"]
    docs += [("abc"[i % 3] + DROP[f][i % 4]) for i in range(700)]   # B: rows of one id, each ends with a dropped code point
    docs += [(HANGUL + E_ACUTE + " ") * 1500, "z a", DROP[f] * 5]    # ... a last row of dropped code points only
    return Case("C_norm_f7", docs, NORM, "docs", dict(n_rows=len(docs), dropped_rows=[1, 105, len(docs) - 1], min_tiles=3), flags=f)


def names(groups="LSBNC"):
    return [n for n in CASES if n[0] in groups]


@functools.lru_cache(maxsize=8)
def build(name):
    c = CASES[name]()
    assert c.name == name
    return c


# one representative per family for the bounds-checking build and the arena guard
SUBSET = ("L_nl_iter_edges_tile1", "L_8a_cp2_tile", "L_len_T_open", "L_only_nl_T+77", "S_behind_5000_4", "S_consecutive", "S_rows_257",
          "B_bound_2048", "B_empty_300", "N_only_dropped_last_f7", "N_only_dropped_all_1_f1", "N_tiles_hangul_f4", "N_tiles_zwsp_f1",
          "C_plain", "C_norm_f7")
SUBSET_MAX_LENS = (1, 5, 33, 200)
