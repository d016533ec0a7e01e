"""The batches of the repetition tests (test_gpu_repetition.py, test_repetition_abi.py): name -> rows of bytes."""
import numpy as np

WORD_TILE, BYTE_TILE = 256, 2048  # kBlock words of the cover kernel, kQualTile bytes of the class pass
K = [b"k%d" % i for i in range(12)]
G = b"g0 g1 g2 g3 g4 g5 g6 g7 g8 g9"  # a 10-gram
ONE = [bytes([c]) for c in b"abcdefghijklmnopqrstuvwxyz0123456789"]  # words of one character


def join(rows):
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return b"".join(rows), off


def _agree(m):
    """two windows that agree in exactly m leading words, each with a word behind them"""
    return b" ".join(K[:m] + [b"u", b"q"] + K[:m] + [b"v", b"t"])


def _word_edges():
    """a duplicate 10-gram that begins at every offset from -10 to +1 around a tile edge of the cover kernel"""
    rows, g = [], 0
    for d in range(-10, 2):
        f = (d - (g + 10)) % WORD_TILE or WORD_TILE
        rows.append(G + b" " + b" ".join(b"f%dx%d" % (d + 10, i) for i in range(f)) + b" " + G + b" end")
        g += 10 + f + 11
    return rows


def _byte_edges():
    """... and of the class pass: one filler word puts the second 10-gram's first byte there"""
    rows, g = [], 0
    for d in range(-10, 2):
        f = (d - (g + len(G) + 2)) % BYTE_TILE or BYTE_TILE
        rows.append(G + b" " + (b"%02d" % (d + 10)) * (f // 2) + b"x" * (f % 2) + b" " + G)
        g += len(rows[-1])
    return rows


def _random(seed, n_rows=200, most=40):
    rng = np.random.default_rng(seed)
    alphabet, gaps = [b"a", b"bb", "çcc".encode()], [b" ", b"  ", b"\t", b"\n"]
    return [b"".join(alphabet[rng.integers(3)] + gaps[rng.integers(4)] for _ in range(rng.integers(most + 1))) for _ in range(n_rows)]


def _rule_rows():
    """row k: rule k at equality: an n-gram twice among 4 n characters (limit 500), its second occurrence among them (250)"""
    return [b" ".join(ONE[:n] * 2 + ONE[n:3 * n]) for n in range(2, 11)]


RULES_AT = {("max_top_%d_chars" if n < 5 else "max_dup_%d_chars") % n: 500 if n < 5 else 250 for n in range(2, 11)}
A33, A300 = b"x" * 32, b"y" * 299
CASES = {
    "row sizes": lambda: [r for k in list(range(13)) + [30] for r in (b" ".join([b"w"] * k), b"", b" ".join(K[:k]))],
    "seam": lambda: [b"a b c d e f", b"a b c d e f", b"a b c d e f a b c d e f", b"", b"a b c d e f"],
    "thrice": lambda: [b"a b c d e x a b c d e y a b c d e", b"a b c a b c a b c"],
    "agree": lambda: [_agree(m) for m in range(1, 12)],
    "ties": lambda: [b"aa bb aa bb c d c d", b"c d c d aa bb aa bb", b"ab cd ab cd ef gh ef gh", b"a b a b a b cc dd cc dd"],
    "spacing": lambda: [b"a  b a\tb", b"ab c a bc", b"ab c ab c", b"a,b a ,b a , b", b" \n a b \n a b \n "],
    "multibyte": lambda: ["été über été über naïve été über".encode(), "日本語".encode() * 5,
                          b"a\xff b a\xff b a\xfe b \xe6\x97 c \xe6\x97 c"],
    "long words": lambda: [b" ".join([A33 + b"a", A33 + b"b", A33 + b"a", A33 + b"b", A33 + b"a", A33 + b"c"]),
                           b" ".join([A300 + b"a", b"z"] * 3 + [A300 + b"b", b"z"] * 3)],
    "word tile edges": _word_edges,
    "byte tile edges": _byte_edges,
    "three tiles": lambda: [b"x y", b" ".join([b"a", b"bb", b"c"][i] for i in np.random.default_rng(3).integers(3, size=2400)), b"x y x y"],
    "random 0": lambda: _random(0),
    "random 1": lambda: _random(1),
    "random 2": lambda: _random(2),
    "rules": _rule_rows,
}
