"""Constructed batches for the line filter, by name: CASES[name]() -> (rows, keywords of the filter call).  T is the byte
tile of the phrase scan and of the cut; nothing exceeds three tiles."""
import random

import numpy as np

T = 2048
C4ISH = {"min_words": 2, "not_terminal": 0}
TERMINAL = {"not_terminal": 0}


def join(rows):
    return b"".join(rows), np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)


def fill(n):
    """n >= 1 bytes of words without a line feed, the last one a full stop"""
    return (b"so it goes. " * (n // 12 + 1))[:n - 1] + b"."


def _at(shift, phrase=b"spam"):
    """one row with the phrase at byte `shift`, and lines around it"""
    return lambda: ([fill(shift - 1) + b"\n" + phrase + b" is here.\n" + fill(300) + b"\nmore " + phrase + b"\n"], dict(phrases=[phrase], rules=TERMINAL))


def _bounded():
    sides = (b"", b"a", b"7", b"\xc3\xa9", b".", b" ", b"Z")
    return [f + b"ass" + b for f in sides for b in sides] + [b"An ass.\nclass pass\n(ass) 1ass ass1"], dict(phrases=[b"ass"], doc_phrases=[b"ss"], bounded=True)


def _dups(scope, min_chars=0):
    rows = [b"x y z.\nx y z.\nu v.\n", b"x y z.\nq.\n\nq.", b"u v.", b"u v.\nu v.", b"", b"x y z."]
    return lambda: (rows, dict(dup_scope=scope, dup_min_chars=min_chars))


def _cut_phase(k):
    return lambda: ([b"D" * (k + 1) + b"\n" + fill(T - 40) + b"\nbad line\n" + fill(T + 7) + b"\n", b"ok.\n"], dict(rules=TERMINAL))


def _random(seed):
    def make():
        rng = random.Random(seed)
        rows = [bytes(rng.choice(b"ab .\nA") for _ in range(rng.choice((0, 1, 3, 9, 20, 33)))) for _ in range(300)]
        return rows, dict(phrases=[b"ab", b"b.", b"a "], doc_phrases=[b"a", b"ba b"], rules={"min_words": 2, "min_chars": 4, "min_kept_lines": 1, "max_doc_phrase_hits": 6},
                          dup_scope=1 + seed % 2, dup_min_chars=2)
    return make


CASES = {
    "match ends on tile end": _at(T - 4),
    "match starts on tile end": _at(T - 1),
    "match across the second tile end": _at(2 * T - 2, b"privacy policy"),
    "tail reaches the batch end": lambda: ([fill(100) + b"\n" + b"q" * 32, fill(T - 164) + b"q" * 31 + b"Q"], dict(phrases=[b"q" * 32], doc_phrases=[b"q" * 31])),
    "cut by a row end": lambda: ([b"this is spa", b"m and more spam", b"spa"], dict(phrases=[b"spam"], doc_phrases=[b"pam"])),
    "one byte phrases": lambda: ([b"ab}", b"cd}\n}", b"}"], dict(phrases=[b"}"], doc_phrases=[b"}", b"d"])),
    "shared prefix": lambda: ([b"a cookie.\na cook.\na co.\nCOOKIES\n"], dict(phrases=[b"cookie", b"cook"], doc_phrases=[b"coo", b"co", b"c"])),
    "upper case": lambda: ([b"Enable JavaScript now.\nJAVASCRIPT\njava script\n"], dict(phrases=[b"javascript"])),
    "multibyte": lambda: (["Un café noir.\nCAFÉ\ncafe\n日本語 text.\n".encode()], dict(phrases=["café".encode(), "本".encode()], doc_phrases=[b"\xa9 n", b"\x00"])),
    "bounded": _bounded,
    "a wave of matches": lambda: ([b"{abcdef " * 64 + b"\n" + fill(T - 513 - 9) + b"{", b"{" * 600, fill(700)], dict(doc_phrases=[b"{"], phrases=[b"{{{"])),
    "document phrase in a dropped line": lambda: ([b"lorem ipsum\nA good line here.\n"], dict(doc_phrases=[b"lorem ipsum"], rules=dict(C4ISH, max_doc_phrase_hits=0))),
    "a phrase listed twice": lambda: ([b"spam spam.\nham.\n"], dict(phrases=[b"spam", b"spam"], doc_phrases=[b"ham", b"ham"])),
    "short rows": lambda: ([b"", b"a", b"a\n", b"\n", b"\n\n\n", b"\n\na b c.\n\nd e f\n\n", b"last line no feed", b"   \nx y z.\n \n", b"a b!", b"..."],
                           dict(rules=dict(C4ISH, min_chars=3, ellipsis_end=0, min_kept_lines=1, min_kept_words=3))),
    "three tiles": lambda: ([b"Short one.\n" + fill(2 * T + 300)[:-1] + b"x\nKept two.\n", fill(2 * T + 100) + b"\nbad\n"], dict(rules=TERMINAL)),
    "many lines": lambda: ([b"a\n" * 1500, b"\n" * 50] + [b"a", b"b."] * 1300, dict(dup_scope=1, phrases=[b"b"], rules={"min_kept_lines": 1})),
    "dups off": _dups(0), "dups in a row": _dups(1), "dups in the batch": _dups(2), "dups at the chars": _dups(2, 6), "dups above the chars": _dups(2, 7),
    "cut phase 0": _cut_phase(0), "cut phase 1": _cut_phase(1), "cut phase 2": _cut_phase(2), "cut phase 3": _cut_phase(3),
    "cut rows": lambda: ([b"bad\nGood one.\nbad", b"bad\nbad", b"Good one.\nGood two.\n", b"\n\nbad\n\n", b"\n"], dict(rules=TERMINAL)),
    "compact drops the ends": lambda: ([b"bad", b"Good.\nbad\n", b"bad\n"], dict(rules=dict(TERMINAL, min_kept_lines=1))),
    "compact drops every row": lambda: ([b"bad", b"bad\n"], dict(rules=dict(TERMINAL, min_kept_lines=1))),
    "random 0": _random(0), "random 1": _random(1),
}
HARD = ("match starts on tile end", "a wave of matches", "short rows", "three tiles", "many lines", "dups in a row", "cut phase 1", "random 0")
