"""The cases of tests/test_gpu_quality.py: rows built around the geometry of the class pass (quality.h) — what straddles
a tile edge, what a row boundary cuts, rows that are empty or one byte long, one long row beside many short ones,
duplicate lines of every kind, and a small corpus for the rules and the presets."""
import numpy as np

T = 2048      # bytes per workgroup of the class pass (quality.h: kQualTile)
SLOTS = 32    # rows of a tile whose sums meet in LDS (kQualSlots)
CHUNK = 256   # bytes per chunk of the duplicate-row search (dedup.h)

# what must not break at an edge: a word, a run of dots, U+2026, U+2022 behind a line feed, characters of 2, 3 and 4
# bytes, a line feed pair, an invalid sequence, a stop word in upper case
STRADDLERS = [b"Word", b"...", b"....", "…".encode(), "\n• x".encode(), "é".encode(), "中".encode(), "\U0001F600".encode(), b"\n\n", b"\xe2\x80", b"\xf0\x9f\x98",
              b" THE ", b"#", b"x!\n", b" \n"]
FILL = "ab c. de\nThe 7 of - 中é,\n".encode()


def filler(n, phase=0):
    reps = (n + phase) // len(FILL) + 2
    return (FILL * reps)[phase:phase + n]


def join(rows):
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    if rows:
        off[1:] = np.cumsum([len(r) for r in rows])
    return b"".join(rows), off


def tile_edge_rows():
    """rows of exactly 3 T bytes (so every row starts at a tile edge), each with one straddler across both inner edges at
    every split of its bytes"""
    rows = []
    for x in STRADDLERS:
        for cut in range(len(x) + 1):
            row = bytearray(filler(3 * T, phase=len(rows) % 7))
            for edge in (T, 2 * T):
                row[edge - cut:edge - cut + len(x)] = x
            assert len(row) == 3 * T
            rows.append(bytes(row))
    return rows


def row_boundary_rows():
    """every straddler cut by a row boundary at every split, the boundary at every byte phase of a word"""
    rows = []
    for x in STRADDLERS:
        for cut in range(len(x) + 1):
            lead = filler(5 + (len(rows) // 2) % 9, phase=len(rows) % 5)
            rows.append(lead + x[:cut])
            rows.append(x[cut:] + filler(3 + len(rows) % 4))
    return rows


def empty_and_single_rows():
    singles = [bytes([b]) for b in (0x61, 0x0A, 0x20, 0x2E, 0x23, 0x2D, 0xFF, 0x80, 0xE2, 0x41, 0x37, 0x21)]
    return [b"", b""] + singles[:6] + [b"", b"", b""] + singles[6:] + [b"", b"a b", b""]


def long_beside_short(rng):
    short = [filler(int(n), phase=int(p)) for n, p in zip(rng.integers(0, 8, 1000), rng.integers(0, 20, 1000))]
    return short[:500] + [filler(3 * T + 5, phase=3)] + short[500:]


def space_lines_rows():
    return [b"   \n\t\t\n a \n", " \n▁▁\nx".encode(), b"\n\n\n", b" ", b"  \n  \n  "]


def duplicate_rows():
    long_a = b"q" * (CHUNK - 1)
    rows = [
        b"same line\nother\n", b"same line\n",                       # equal lines in different rows: no duplicate
        b"rep\nrep\nx\nrep\n",                                       # three times: 2
        b"tail\nmid\ntail",                                          # the last line without a line feed
        long_a + b"A\n" + long_a + b"B\n" + long_a + b"A\n",         # differ only in the last byte of the first chunk
        b"z" * (3 * CHUNK + 7) + b"1\n" + b"z" * (3 * CHUNK + 7) + b"2\n" + b"z" * (3 * CHUNK + 7) + b"1",   # beyond 3 chunks
        b"a\n\nb\n\na\n\n\nb",                                       # separator runs of line feeds between duplicate lines
        b"\n\nx\n\n",                                                # a row that begins and ends with separators
        "中 é\n中 é\n".encode() + b"\xff\xe4\n\xff\xe4\n",              # the characters of a duplicate line, of valid and of invalid bytes
        b"", b"only",
        b"r" * (CHUNK + 24) + b"A\n" + b"r" * (CHUNK + 24) + b"B\n" + b"r" * (CHUNK + 24) + b"A\n",   # differ only beyond the first chunk (byte 280)
    ]
    return rows


def corpus(rng):
    """documents of several kinds for the rules and the presets: prose with stop words, bullet lists, code-like rows with
    hashes, ellipsis-heavy rows, rows of duplicate lines, rows of symbols"""
    words = ["the", "of", "and", "to", "that", "with", "have", "be", "model", "quality", "filter", "corpus", "Data", "GPU", "x", "中文", "naïve", "2024", "a1"]

    def sentence(n):
        return " ".join(words[i] for i in rng.integers(0, len(words), n)).capitalize() + rng.choice([".", "!", "?", "", "...", "…"])
    docs = []
    for k in range(60):
        kind = k % 6
        n_lines = int(rng.integers(1, 12))
        if kind == 0:
            lines = [sentence(int(rng.integers(3, 18))) for _ in range(n_lines)]
        elif kind == 1:
            lines = [rng.choice(["- ", "• ", "* "]) + sentence(int(rng.integers(1, 6))) for _ in range(n_lines)]
        elif kind == 2:
            lines = ["# " + sentence(2) + " ## #" if rng.random() < 0.5 else sentence(4) for _ in range(n_lines)]
        elif kind == 3:
            lines = [sentence(3) + "..." for _ in range(n_lines)]
        elif kind == 4:
            base = [sentence(5) for _ in range(3)]
            lines = [base[int(rng.integers(0, 3))] for _ in range(n_lines)]
        else:
            lines = ["".join(rng.choice(list("!@$%^&*()[]{}<>1234567890")) for _ in range(int(rng.integers(1, 40)))) for _ in range(n_lines)]
        docs.append(("\n".join(lines) + ("\n" if rng.random() < 0.7 else "")).encode())
    # rows with exact ratios for the rules at equality: 8 words with 3 hashes, 4 lines with 1 bullet / ellipsis / terminal / duplicate ...
    docs += [b"# # # a b c d e", b"- a\nb\nc\nd", b"a...\nb\nc\nd", b"a.\nb\nc\nd", b"a\na\nc\nd", b"a ... b c d e f g", b"the of a b c d e f",
             b"ab\nab\ncdcd\nefef\n", b"x" * 31 + b"\nb\nc\nd", b"a b\nc d\ne f\ng h\n", b"1 2 3 a b c d e", b"abcd ef"]
    return docs
