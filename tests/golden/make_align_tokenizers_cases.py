"""Writes tests/golden/align_tokenizers_cases.json: seeded (text, answer) cases over one small vocabulary, with the
character offsets a `tokenizers` BERT WordPiece pipeline gives the text and what its Encoding.char_to_token says of the
answer's first and last character (None where that character lies in no token).  Needs the `tokenizers` package; the
fixture pins its behaviour where the package is absent (tests/test_align_model.py)."""
import json
import os
import random

import tokenizers
from tokenizers import Tokenizer, models, normalizers, pre_tokenizers

VOCAB = ["[UNK]", "[CLS]", "[SEP]", "[PAD]", "a", "b", "c", "ab", "abc", "##a", "##b", "##c", "##ab", "##bc", "foo", "##oo", "bar",
         "##r", ".", ",", "-", "é", "##é", "中", "hello", "##s", "world", "x", "##x", "Paris", "France", "of", "the", "capital", "is"]
WORDS = ["a", "b", "c", "ab", "abc", "abcab", "aab", "foo", "fooa", "bar", "barr", "é", "aé", "éé", "中", "hello", "hellos", "world",
         "x", "xx", "Paris", "France", "of", "the", "capital", "is", "zebra", "q"]
SEPS = [" ", " ", " ", "  ", ".", ", ", "-", " . ", "\n", "中"]


def make_tokenizer():
    tok = Tokenizer(models.WordPiece({w: i for i, w in enumerate(VOCAB)}, unk_token="[UNK]"))
    tok.normalizer = normalizers.BertNormalizer(clean_text=False, handle_chinese_chars=True, strip_accents=False, lowercase=False)
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    return tok


def random_text(rng):
    parts = []
    for _ in range(rng.randint(1, 14)):
        parts.append(rng.choice(WORDS))
        parts.append(rng.choice(SEPS))
    if rng.random() < 0.5:
        parts.pop()
    if rng.random() < 0.2:
        parts.insert(0, rng.choice((" ", "  ")))
    return "".join(parts)


def record(tok, text, begin, end):
    e = tok.encode(text, add_special_tokens=False)
    return {"text": text, "offsets": [list(o) for o in e.offsets], "answer": [begin, end], "first": e.char_to_token(begin),
            "last": e.char_to_token(end - 1)}


def main():
    rng = random.Random(20261020)
    tok = make_tokenizer()
    cases, seen = [], set()
    fixed = [("Paris is the capital of France.", 0, 5), ("Paris is the capital of France.", 24, 30), ("Paris is the capital of France.", 9, 20),
             ("hellos world", 5, 6), ("hellos world", 0, 12), ("a  b", 1, 3), ("abcab", 2, 4), ("é中é", 1, 2), ("zebra foo", 0, 5)]
    while len(cases) < 400:
        if len(cases) < len(fixed):
            text, begin, end = fixed[len(cases)]
        else:
            text = random_text(rng)
            begin = rng.randrange(len(text))
            end = rng.randint(begin + 1, min(len(text), begin + rng.choice((1, 2, 5, 12, 40))))
        if (text, begin, end) in seen or not tok.encode(text, add_special_tokens=False).ids:
            continue
        seen.add((text, begin, end))
        cases.append(record(tok, text, begin, end))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "align_tokenizers_cases.json")
    with open(path, "w") as f:
        json.dump({"tokenizers": tokenizers.__version__, "vocab": VOCAB, "cases": cases}, f, ensure_ascii=True, indent=0)


if __name__ == "__main__":
    main()
