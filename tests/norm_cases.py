"""Inputs placed on the seams of the normalise pre-pass (csrc/normalize.h: norm_count_kernel, norm_write_kernel and its
row flush, span_source_kernel; the word-wide ASCII helpers in csrc/utf8_swar.h), shared by test_norm_cases.py (no GPU) and
test_gpu_norm_edges.py: the layout constants, read from the headers by name; a plain-Python layout model over
normalize_model.normalize and offsets_model.decode_with_starts that says, per 1 KB row and lane, which of the four ways an
ASCII byte can take the lane's chunk goes

  row    every lane's chunk of the row is 16 bytes of the text, all below 0x80, none dropped by WP_NORM_CLEAN: the row is
         lowered with word-wide arithmetic and copied (row_simple);
  lane   the lane's chunk is such a chunk inside a row that is not (lane_simple);
  lean   norm_chunk with no ASCII byte of the chunk dropped: ASCII copied between the leads that go through the rule;
  rule   norm_chunk with an ASCII control dropped: every code point goes through norm_cp;

what the row gives (bytes, normalised and source code points), at which output position and so at which alignment
a = out & 3 it is flushed, and per tile the three sums the scans carry; and the cases, in groups

  A  every ASCII value through each path, at each of the 16 byte positions of a chunk ("kept": the values WP_NORM_CLEAN
     keeps, so that the paths are reached under the flag sets with it; "all": all 128, for the flag sets without);
  T  the whole code space, at every word phase;
  X  rows that give 0, 1, 2, 3, 4, 5, 7, 8 bytes at each output alignment, as row 3 of a wave, as the last row of a tile and
     as the ragged end; the rows that give the most; tiles and texts that give nothing;
  S  a code point that shrinks, grows or vanishes under the rule, 1, 2, 3 bytes in front of a chunk, row, wave or tile
     boundary, cut short by the end of the text, or replaced by an invalid look-alike;
  M  the source map, entry by entry, through single_symbol_vocab;
  F  100 seeded compositions of the same building blocks at random row phases;
  H  sequences of calls on one handle (SEQUENCES).

build(name) -> (text bytes, expect).  expect["claims"] is what the builder says it built; test_norm_cases.py holds the layout
model to it.  Claims that depend on the flag set are dicts keyed by the flag set and hold only for the flag sets they name.
Importing this module loads no library."""
import itertools
import os
import random
import re

import normalize_model as NM
import offsets_model as OM
from bruteforce import is_space
from decode_cases import CHUNK, CSRC, LANES, ROW, TILE, WAVE, _constant


def _row_out():
    """kNormRowOut = 3 * (kDecRowBytes + 4), read from normalize.h by name (the factors are part of the header's line)"""
    assert _constant("decode.h", "kDecChunk") * LANES == ROW
    with open(os.path.join(CSRC, "normalize.h")) as f:
        m = re.search(r"^constexpr\s+int\s+kNormRowOut\s*=\s*(\d+)\s*\*\s*\(kDecRowBytes\s*\+\s*(\d+)\)\s*;", f.read(), re.M)
    assert m, "kNormRowOut"
    return int(m.group(1)) * (ROW + int(m.group(2)))


ROW_OUT = _row_out()
ROWS_PER_TILE = TILE // ROW
MAX_TEXT = 3 * TILE + ROW
ALL_FLAGS = tuple(range(8))
CLEAN_FLAGS = tuple(f for f in ALL_FLAGS if f & NM.CLEAN)
PLAIN_FLAGS = tuple(f for f in ALL_FLAGS if not f & NM.CLEAN)
MAP_FLAGS = (1, 4, 7)

_CACHES = {f: {} for f in ALL_FLAGS}


def model(text, flags):
    """normalize_model.normalize with one cache per flag set (flags 0: every valid code point is itself)"""
    return NM.normalize(text, flags, _CACHES[flags])


def _utf8_len(c):
    return 1 if c < 0x80 else 2 if c < 0x800 else 3 if c < 0x10000 else 4


# ---- the layout model -------------------------------------------------------------------------------------------------------

class Layout:
    """What the two passes make of (text, flags).  norm / src_byte / src_cp: normalize_model.normalize.  Per row r that holds
    a byte of the text rows[r] = dict(base, paths=[per lane "row" / "lane" / "lean" / "rule" / None (no byte of the text)],
    nb / nc / sc = bytes and code points the row gives and valid code points of the source whose lead it holds, out = output
    byte of its first one, a = out & 3); tiles[t] = (nb, nc, sc) summed over the tile's rows."""

    def __init__(self, text, flags):
        self.text, self.flags, self.nbytes = text, flags, len(text)
        self.norm, self.src_byte, self.src_cp = model(text, flags)
        self.cps, self.starts = OM.decode_with_starts(text)
        cache = _CACHES[flags]
        dropped = [c for c in range(0x80) if not cache.setdefault(c, NM.normalize_cp(flags, c))]
        is_dropped = bytearray(256)
        for c in dropped:
            is_dropped[c] = 1
        self.rows = []
        n_rows = (len(text) + ROW - 1) // ROW
        acc = [[0, 0, 0] for _ in range(n_rows)]
        for c, s in zip(self.cps, self.starts):
            img = cache[c]
            a = acc[s // ROW]
            a[0] += sum(map(_utf8_len, img))
            a[1] += len(img)
            a[2] += 1
        out = 0
        for r in range(n_rows):
            base = r * ROW
            paths = []
            for lane in range(LANES):
                chunk = text[base + lane * CHUNK:base + (lane + 1) * CHUNK]
                if not chunk:
                    paths.append(None)
                    continue
                drops = any(is_dropped[b] for b in chunk if b < 0x80)
                simple = len(chunk) == CHUNK and max(chunk) < 0x80 and not drops
                paths.append("lane" if simple else "rule" if drops else "lean")
            if all(p == "lane" for p in paths):
                paths = ["row"] * LANES
            nb, nc, sc = acc[r]
            self.rows.append(dict(base=base, paths=paths, nb=nb, nc=nc, sc=sc, out=out, a=out & 3))
            out += nb
        assert out == len(self.norm)
        self.tiles = [tuple(sum(r[k] for r in self.rows[t:t + ROWS_PER_TILE]) for k in ("nb", "nc", "sc"))
                      for t in range(0, n_rows, ROWS_PER_TILE)]

    def path_at(self, byte):
        return self.rows[byte // ROW]["paths"][byte % ROW // CHUNK]

    def source_of_output_byte(self, k):
        """the byte of the text whose code point gave byte k of the normalised text"""
        pos = 0
        for q, c in enumerate(OM.decode_with_starts(self.norm)[0]):
            pos += _utf8_len(c)
            if k < pos:
                return self.src_byte[q]
        return self.nbytes


def describe(text, flags, k):
    """where byte k of the normalised text comes from, for a failure message"""
    m = Layout(text, flags)
    s = m.source_of_output_byte(k)
    if s >= len(text):
        return "output byte %d: behind the model's text (%d bytes)" % (k, len(m.norm))
    return "output byte %d <- source byte %d (row %d, lane %d, path %s)" % (k, s, s // ROW, s % ROW // CHUNK, m.path_at(s))


# ---- vocabularies -----------------------------------------------------------------------------------------------------------

def single_symbol_vocab(text, flags):
    """[UNK] and, for every non-blank code point of the model-normalised text, the code point and its "##" form: an
    encode gives one id per non-blank normalised code point"""
    cps = sorted({c for c in OM.decode_with_starts(model(text, flags)[0])[0] if not is_space(c)})
    return ["[UNK]"] + [chr(c) for c in cps] + ["##" + chr(c) for c in cps]


# ---- building blocks --------------------------------------------------------------------------------------------------------
E2, C3, C4 = "é".encode(), "中".encode(), "😀".encode()
FILL = b"aB ,.-\t\n@[`{Zz~Q"   # both cases, the values next to A, Z, a, z, blanks: a byte one position off differs from its neighbour
VANISH = "\u200b\u00ad\u0001".encode()   # 3 + 2 + 1 bytes that WP_NORM_CLEAN drops and no other flag touches
HANGUL_ROW = "각" * 342              # 1026 bytes -> 3078 under WP_NORM_STRIP_ACCENTS: the documented maximum of a row
NOTE_ROW = "\U0001d160" * 256            # 1024 bytes -> 3072
NEIGHBOURS = (0x08, 0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x0E, 0x1F, 0x20, 0x40, 0x41, 0x5A, 0x5B, 0x60, 0x61, 0x7A, 0x7B, 0x7E, 0x7F)
KEPT = {f: tuple(c for c in range(0x80) if NM.normalize_cp(f, c)) for f in ALL_FLAGS}
assert len(KEPT[0]) == 128 and len(KEPT[1]) == 98 and KEPT[1] == KEPT[7]


def fill(n, seed):
    return bytes(random.Random(seed).choices(FILL, k=n))


def vanishing(n):
    """n bytes that give nothing under WP_NORM_CLEAN"""
    return VANISH * (n // 6) + b"\x01" * (n % 6)


def giving(n_src, n_out, seed=0):
    """n_src bytes that give exactly n_out bytes under WP_NORM_CLEAN: letters spread over code points that vanish"""
    rest = n_src - n_out
    cps = [VANISH[:3], VANISH[3:5], VANISH[5:]] * (rest // 6) + [b"\x01"] * (rest % 6)
    for i in range(n_out):
        cps.insert((i + 1) * len(cps) // (n_out + 1) + i, bytes([0x41 + (seed + 7 * i) % 26 + 0x20 * (i & 1)]))
    out = b"".join(cps)
    assert len(out) == n_src
    return out


def compose(n_chunks, plan, stream):
    """n_chunks chunks: plan(i) = None or (position in the chunk, bytes) puts `bytes` there (it may reach into the next
    chunk), every other byte is the next of `stream`"""
    out = bytearray()
    for i in range(n_chunks):
        item = plan(i)
        if item is not None:
            pos, seq = item
            assert len(out) <= i * CHUNK + pos, (i, item)
            while len(out) < i * CHUNK + pos:
                out.append(next(stream))
            out += seq
        while len(out) < (i + 1) * CHUNK:
            out.append(next(stream))
    return bytes(out)


CASES = {}       # name -> (text or its maker, expect)
SEQUENCES = {}   # name -> [(call, text, flags, ...)] (group H)


def later(f, *args, **kw):
    return lambda: f(*args, **kw)


def _add(name, text, **claims):
    assert name not in CASES, name
    CASES[name] = (text, dict(claims=claims))


# ---- A: every ASCII value through each path -----------------------------------------------------------------------------------
# a cycle of odd period over the values: after period x 16 bytes every value has stood at every position of a chunk
A_VALUES = {"kept": KEPT[1] + (0x61,), "all": tuple(range(128)) + (0x61,)}
assert all(len(v) % 2 == 1 for v in A_VALUES.values())
A_ROWS = {"row": 3, "lane": 3, "lean": 12, "rule": 8}
A_LEAN_PLAN = [(0, E2), (0, C3), (0, C4), (7, E2), (7, C3), (7, C4), (15, E2), (15, C3), (15, C4), (7, E2)]


def _a_text(kind, values, lane=None):
    stream = itertools.cycle(A_VALUES[values])
    n = A_ROWS[kind] * LANES
    if kind == "row":
        return compose(n, lambda i: None, stream)
    if kind == "lane":   # one é in the middle of lane `lane` of every row
        return compose(n, lambda i: (0, b"a" * 7 + E2 + b"a" * 7) if i % LANES == lane else None, stream)
    if kind == "lean":   # a 2, 3, 4-byte code point at chunk position 0, in the middle, with its lead at byte 15
        return compose(n, lambda i: A_LEAN_PLAN[i % len(A_LEAN_PLAN)], stream)
    # U+0001 at a position that moves through the chunk, beside each ASCII value in turn (a cycle of period 131: a prime)
    stream = itertools.cycle(tuple(range(128)) + (0x61, 0x62, 0x63))
    return compose(n, lambda i: (i % CHUNK, b"\x01"), stream)


def _a_claims(kind, values, lane=None):
    """paths[f]: the path of every chunk of the full rows (lane cases: of every chunk but lane `lane`'s, which is lean);
    covers[f]: every value of KEPT[f] stands at each of the 16 positions of a chunk of that path"""
    flags = ALL_FLAGS if values == "kept" else PLAIN_FLAGS
    covers = CLEAN_FLAGS if values == "kept" else PLAIN_FLAGS
    if kind == "rule":
        paths = {f: "rule" if f & NM.CLEAN else "row" for f in ALL_FLAGS}
        return dict(paths=paths, covers=ALL_FLAGS, covers_all_values=True, neighbours=NEIGHBOURS, rows=A_ROWS[kind])
    paths = {f: kind for f in flags}
    return dict(paths=paths, covers=covers, neighbours=NEIGHBOURS, lane=lane, rows=A_ROWS[kind])


for _values in ("kept", "all"):
    _add("A_row_%s" % _values, later(_a_text, "row", _values), **_a_claims("row", _values))
    for _lane in (0, 31, 63):
        _add("A_lane_%d_%s" % (_lane, _values), later(_a_text, "lane", _values, _lane), **_a_claims("lane", _values, _lane))
    _add("A_lean_%s" % _values, later(_a_text, "lean", _values), **_a_claims("lean", _values))
_add("A_rule", later(_a_text, "rule", "all"), **_a_claims("rule", "all"))


# ---- T: the whole code space ----------------------------------------------------------------------------------------------------
T_SHIFTS = (0, 1, 2, 3)
T_BYTES = 128 + 2 * (0x800 - 0x80) + 3 * (0x10000 - 0x800 - 0x800) + 4 * 0x100000


def t_scalars():
    return itertools.chain(range(0xD800), range(0xE000, 0x110000))


def t_text(shift):
    """every scalar value in order, behind `shift` ASCII bytes"""
    return b"x" * shift + "".join(map(chr, t_scalars())).encode("utf8")


def t_images(flags):
    """per scalar value, in order: the UTF-8 of what it gives (2.3 s per flag set: build once per module)"""
    if flags == 0:
        return [chr(c).encode("utf8") for c in t_scalars()]
    return ["".join(map(chr, NM.normalize_cp(flags, c))).encode("utf8") for c in t_scalars()]


def t_first_difference(got, images, shift):
    """the first scalar value whose image is not where the expectation has it -> a message"""
    pos = shift
    if got[:shift] != b"x" * shift:
        return "the %d ASCII bytes in front differ" % shift
    for c, img in zip(t_scalars(), images):
        if got[pos:pos + len(img)] != img:
            return "U+%04X: expected %s at output byte %d, got %s" % (c, img.hex() or "nothing", pos, got[pos:pos + max(len(img), 4)].hex())
        pos += len(img)
    return "%d bytes behind the last code point" % (len(got) - pos) if len(got) != pos else None


# ---- X: rows that grow, shrink and vanish ---------------------------------------------------------------------------------------
X_GIVES = (0, 1, 2, 3, 4, 5, 7, 8)
X_PLACES = {"wave": 3, "tile": ROWS_PER_TILE - 1, "ragged": 3}   # the row of the text that holds the probe row
X_RAGGED = 701


def _aligned_prefix(rows, a, seed):
    """`rows` rows of ASCII that give rows x ROW - k bytes under WP_NORM_CLEAN, k = (-a) & 3: what follows is written at
    alignment a.  The k dropped controls stand in row 0."""
    b = bytearray(fill(rows * ROW, seed))
    for i in range((-a) & 3):
        b[100 + 200 * i] = 0x01
    return bytes(b)


def _x_text(n, a, place):
    r = X_PLACES[place]
    head = _aligned_prefix(r, a, 10 * n + a)
    if place == "ragged":
        return head + giving(X_RAGGED, n, n)
    return head + giving(ROW, n, n) + fill(ROW + 33, 500 + n)


for _n in X_GIVES:
    for _a in range(4):
        for _place, _r in X_PLACES.items():
            _rows = {_r: (_n, _a)}
            if _place != "ragged":
                _rows[_r + 1] = (ROW, (_a + _n) & 3)
            _add("X_gives%d_a%d_%s" % (_n, _a, _place), later(_x_text, _n, _a, _place),
                 rows={f: _rows for f in CLEAN_FLAGS}, row_paths={f: {_r + 1: "row"} for f in CLEAN_FLAGS if _place != "ragged"},
                 nbytes=_r * ROW + (X_RAGGED if _place == "ragged" else 2 * ROW + 33))


def _x_max_text(row, a):
    """row 0 sets the alignment, row 1 vanishes, row 2 gives the most a row can, the two rows behind are ASCII (the first
    of them behind the bytes the last code point reaches into it)"""
    body = row.encode()
    return _aligned_prefix(1, a, 40 + a) + vanishing(ROW) + body + fill(3 * ROW - len(body), 44 + a)


for _a in range(4):
    _add("X_hangul_a%d" % _a, later(_x_max_text, HANGUL_ROW, _a), nbytes=5 * ROW,
         rows={f: {1: (0, _a), 2: (3078, _a), 3: (ROW - 2, (_a + 3078) & 3), 4: (ROW, (_a + 3078 + ROW - 2) & 3)} for f in (5, 7)},
         row_paths={f: {4: "row"} for f in (5, 7)}, max_row=3078)
    _add("X_note_a%d" % _a, later(_x_max_text, NOTE_ROW, _a), nbytes=5 * ROW,
         rows={f: {1: (0, _a), 2: (3072, _a), 3: (ROW, _a & 3)} for f in (5, 7)}, row_paths={f: {3: "row"} for f in (5, 7)}, max_row=3072)


def _x_tile_text(empty):
    tiles = [fill(TILE - 9, 60 + t) + "é中😀".encode() for t in range(3)]
    tiles[empty] = vanishing(TILE)
    return b"".join(tiles) + fill(77, 63)


for _t, _where in enumerate(("front", "between", "behind")):
    _add("X_empty_tile_%s" % _where, later(_x_tile_text, _t), nbytes=3 * TILE + 77,
         tiles={f: {_t: (0, 0)} for f in CLEAN_FLAGS}, tiles_give={f: [t for t in range(4) if t != _t] for f in CLEAN_FLAGS})
X_NOTHING = (1, 15, 16, 17, ROW - 1, ROW, ROW + 1, TILE - 1, TILE, TILE + 1)
for _n in X_NOTHING:
    _add("X_nothing_%d" % _n, later(vanishing, _n), nbytes=_n, norm_len={f: 0 for f in CLEAN_FLAGS})
_add("X_one_byte_last", later(lambda: vanishing(TILE) + b"Z"), nbytes=TILE + 1, norm_len={f: 1 for f in CLEAN_FLAGS},
     tiles={f: {0: (0, 0)} for f in CLEAN_FLAGS})
_add("X_one_byte_first", later(lambda: b"Z" + vanishing(TILE)), nbytes=TILE + 1, norm_len={f: 1 for f in CLEAN_FLAGS},
     tiles={f: {1: (0, 0)} for f in CLEAN_FLAGS})


# ---- S: a code point across a seam, under the rule ------------------------------------------------------------------------------
S_BOUNDARIES = {"chunk": ROW + 7 * CHUNK, "row": 2 * ROW, "wave": WAVE, "tile": TILE}
S_CPS = {"E9up": (0xC9, 4, 1), "angstrom": (0x212B, 4, 1), "hangul": (0xAC01, 4, 9), "note": (0x1D160, 4, 12), "zwsp": (0x200B, 1, 0),
         "idot": (0x130, 2, 3)}   # name -> (code point, a flag set under which it gives ..., ... this many bytes)
S_FOLLOW = {"upper": b"Q", "ctrl": b"\x0b"}
S_INVALID = {"E4B8": b"\xe4\xb8", "F09F98": b"\xf0\x9f\x98", "EDA080": b"\xed\xa0\x80", "C0AF": b"\xc0\xaf"}


def boundary_kind(x):
    return "tile" if x % TILE == 0 else "wave" if x % WAVE == 0 else "row" if x % ROW == 0 else "chunk" if x % CHUNK == 0 else None


def _s_text(X, pos, seq, follow, cut=False):
    head = fill(pos, X + pos) + seq
    return head if cut else head + follow + fill(X + 41 - len(head) - len(follow), X + 1)


for _kind, _X in S_BOUNDARIES.items():
    for _s in (1, 2, 3):
        for _cp_name, (_cp, _f, _gives) in S_CPS.items():
            _seq = chr(_cp).encode()
            for _fname, _follow in S_FOLLOW.items():
                _add("S_%s_s%d_%s_%s" % (_kind, _s, _cp_name, _fname), later(_s_text, _X, _X - _s, _seq, _follow),
                     seam=(_kind, _X, _X - _s), cp=_cp, gives={_f: _gives}, follow=_follow, nbytes=_X + 41)
            # the end of the text cuts the sequence one byte short: nothing of it is left
            _add("S_%s_s%d_%s_cut" % (_kind, _s, _cp_name), later(_s_text, _X, _X - _s, _seq[:-1], b"", True),
                 seam=(_kind, _X, _X - _s), cut=True, nbytes=_X - _s + len(_seq) - 1)
        for _iname, _seq in S_INVALID.items():
            _add("S_%s_s%d_inv_%s" % (_kind, _s, _iname), later(_s_text, _X, _X - _s, _seq, b"Q"),
                 seam=(_kind, _X, _X - _s), invalid=len(_seq), nbytes=_X + 41)


# ---- M: the source map ----------------------------------------------------------------------------------------------------------
def _m_paths():
    """two rows of each of the four paths of A (the values every flag set of MAP_FLAGS keeps, so that they are paths
    under all three... but the rule path, which needs a control that WP_NORM_CLEAN drops)"""
    return _a_text("row", "kept")[:2 * ROW], _a_text("lane", "kept", 31)[:2 * ROW], _a_text("lean", "kept")[:2 * ROW + 2]


_add("M_path_row", later(lambda: _m_paths()[0]), paths={f: "row" for f in MAP_FLAGS}, one_id_per_cp=True)
_add("M_path_lane", later(lambda: _m_paths()[1]), paths={f: "lane" for f in MAP_FLAGS}, lane=31, one_id_per_cp=True)
_add("M_path_lean", later(lambda: _m_paths()[2]), paths={f: "lean" for f in MAP_FLAGS}, one_id_per_cp=True)
_add("M_path_rule", later(lambda: _a_text("rule", "all")[:2 * ROW]), paths={1: "rule", 7: "rule", 4: "row"},
     one_id_per_cp=True)
M_PROBE = "AbÉ c\u200bdÅ 각e\U0001d160 fİg.".encode()


def _m_probe_text(row):
    """tile 0 expands (Hangul under STRIP), tile 1 shrinks ("a" + U+200B under CLEAN): normalised code points, source code
    points and bytes all differ at the probe, which stands in the last row of tile 1 or in the first row of tile 2"""
    t0 = ("각" * (TILE // 3)).encode() + b" "
    t1 = ("a\u200b" * (TILE // 4)).encode()
    head = t0 + t1
    assert len(head) == 2 * TILE
    at = 2 * TILE - ROW + 100 if row == "last_of_tile_1" else 2 * TILE + 100
    body = bytearray(head + ("a\u200b" * (ROW // 2)).encode())
    probe = M_PROBE + b"q" * (-len(M_PROBE) % 4)   # whole "a" + U+200B units are replaced
    body[at:at + len(probe)] = probe
    return bytes(body), at


_M_SUMS_DIFFER = {f: True for f in (1, 7)}
_add("M_probe_last_row_of_tile_1", later(lambda: _m_probe_text("last_of_tile_1")[0]), probe=(2 * TILE - ROW + 100, ROWS_PER_TILE * 2 - 1),
     sums_differ=_M_SUMS_DIFFER, one_id_per_cp=True)
_add("M_probe_first_row_of_tile_2", later(lambda: _m_probe_text("first_of_tile_2")[0]), probe=(2 * TILE + 100, ROWS_PER_TILE * 2),
     sums_differ=_M_SUMS_DIFFER, one_id_per_cp=True)
for _L, _ch in ((2, "é"), (3, "中"), (4, "😀")):
    _add("M_span_ends_in_%d_bytes" % _L, ("ab%s cd%s\u200b x%s" % (_ch, _ch, _ch)).encode(), last_cp_bytes=_L, one_id_per_cp=True)
_add("M_dropped_inside_word", "ab\u200bcd e\u00adf\u0001g".encode(), one_id_per_cp=True, dropped_under_clean=3)
_add("M_dropped_behind_last_kept", "abc\u200b\u00ad de\u0001\u200b".encode(), one_id_per_cp=True, dropped_under_clean=4)
_add("M_dropped_at_text_start", "\u200b\u0001\u00adabc d".encode(), one_id_per_cp=True, dropped_under_clean=3)
_add("M_dropped_at_text_end", "abc d\u0001\u200b\u00ad".encode(), one_id_per_cp=True, dropped_under_clean=3)
M_SPLIT_VOCAB = ["[UNK]", "ᄀ", "##ᅡ", "##ᆨ", "x", "##x"]
_add("M_syllable_split", "x 각 가x".encode(), vocab=M_SPLIT_VOCAB, split_syllable=True)
_add("M_ends_in_third_of_expansion", ("ab " + "각" * 20).encode(), one_id_per_cp=True, ends_in_expansion=True)
_add("M_ends_in_third_of_expansion_row", later(lambda: fill(ROW - 3, 90).replace(b"\t", b" ") + ("각" * 341 + "각").encode()),
     one_id_per_cp=True, ends_in_expansion=True)


# ---- F: seeded compositions -------------------------------------------------------------------------------------------------------
F_COUNT = 100


def _f_text(k):
    rng = random.Random(7100 + k)
    parts, size = [], 0
    budget = rng.choice([300, ROW + 50, 2 * ROW, 3 * ROW + 7, WAVE + 100, WAVE + 100, TILE + ROW, 2 * TILE + 500])
    while size < budget:
        r = rng.random()
        room = budget - size
        if r < 0.25:     # to a random row phase, in clean ASCII
            p = fill(rng.randrange(1, 2 * ROW), rng.random())
        elif r < 0.35:
            p = vanishing(rng.choice([1, 5, 16, ROW - 1, ROW, ROW + 5, WAVE]))
        elif r < 0.45:
            p = giving(rng.choice([64, ROW, ROW + 3]), rng.choice(X_GIVES), k)
        elif r < 0.55:
            p = ("각" * rng.choice([1, 5, 342, 400])).encode()
        elif r < 0.62:
            p = ("\U0001d160" * rng.choice([1, 3, 256, 300])).encode()
        elif r < 0.80:
            p = chr(rng.choice([v[0] for v in S_CPS.values()])).encode() + rng.choice([b"", b"Q", b"\x0b", b"\x7f"])
        elif r < 0.88:
            p = rng.choice(list(S_INVALID.values()) + [b"\xff", b"\x80", b"\xf4\x90\x80\x80"])
        else:
            p = bytes(rng.choices(range(128), k=rng.randrange(1, 200)))
        p = p[:room]
        parts.append(p)
        size += len(p)
    return b"".join(parts)


for _k in range(F_COUNT):
    _add("F_%03d" % _k, later(_f_text, _k), composed=True)


# ---- H: one handle, several calls -----------------------------------------------------------------------------------------------
H_VOCAB = ["[UNK]"] + [c for c in "abeqxyz,."] + ["##" + c for c in "abeqxyz"] + ["ᄀ", "##ᅡ", "##ᆨ", "é", "##é", "中", "##中"]
H_SHARD_K = 5000
H_SHARD_VOCAB = ["[UNK]", "x", "##x", "y", "##y", "z"]


def shard_text(k=H_SHARD_K):
    """the balanced cut of two shards (the middle, all of it being ASCII) lies among the x, 8 bytes in front of U+000B: the
    run of y is 16 bytes shorter than the run of x.  (With two runs of k the middle is byte k + 2, the first y, and the
    rule for U+000B / U+000C would not be reached.)"""
    return b"x" * k + b"\x0b\x0c" + b"y" * (k - 16) + b" z"


def _h_long_then_lead():
    first = fill(3 * ROW + 10, 1) + "中中中".encode() + fill(50, 2)
    second = fill(3 * ROW + 10, 1) + "中".encode()[:1]   # its lead stands where the first text had 中
    return first, second


SEQUENCES["H_lead_where_continuation_bytes_were"] = lambda: [("normalize", t, 7) for t in _h_long_then_lead()] + \
    [("encode", t, 7) for t in _h_long_then_lead()]
SEQUENCES["H_flags_7_2_0_7"] = lambda: [(call, ("AbÉ 각\u200bq,İ. " * 300).encode(), f)
                                         for f in (7, 2, 0, 7) for call in ("normalize", "encode")]
SEQUENCES["H_normalize_encode_normalize"] = lambda: [("normalize", ("AbÉ 각 q. " * 500).encode(), 7),
                                                     ("encode", ("bAÉ 각\u200b e, " * 700).encode(), 7),
                                                     ("normalize", ("AbÉ 각 q. " * 500).encode(), 7),
                                                     ("offsets", ("AbÉ 각 q. " * 100).encode(), 7)]
SEQUENCES["H_grow_between_calls"] = lambda: [(call, t, 7) for t in (("a\u200b" * 3000).encode(), ("각 " * 9000).encode(),
                                                                    ("a\u200b" * 3000).encode()) for call in ("normalize", "offsets")]


def names(groups="AXSM"):
    return [n for n in CASES if n[0] in groups]


GROUP_SIZES = {"A": 11, "X": 119, "S": 264, "M": 16, "F": F_COUNT}   # asserted by test_norm_cases.py


def build(name):
    """-> (text bytes, expect)"""
    text, expect = CASES[name]
    if callable(text):
        text = text()
    assert len(text) <= MAX_TEXT, (name, len(text))
    return text, dict(expect)
