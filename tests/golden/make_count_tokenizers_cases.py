"""Writes tests/golden/count_tokenizers_cases.json: seeded random texts over an alphabet on which the word rule of the
word counts and the `tokenizers` package's BertNormalizer(clean_text=False, handle_chinese_chars=True) + BertPreTokenizer
coincide, each with the words the package splits it into.  Needs the `tokenizers` package; the fixture pins its behaviour
where the package is absent (tests/test_count_model.py)."""
import json
import os
import random

import tokenizers
from tokenizers import normalizers, pre_tokenizers

# ASCII 0x21-0x7E; blank, tab, LF, CR; Latin-1 / Cyrillic / kana / Hangul letters; CJK from each is_chinese range; and the
# punctuation outside ASCII that both sides know (the package's sixth range starts at U+2B920, not U+2B820: from there on)
ALPHABET = ([chr(c) for c in range(0x21, 0x7F)] + [" ", " ", " ", "\t", "\n", "\r"] + list("éüñÀøжЩяかなカナ한글")
            + [chr(c) for c in (0x4E00, 0x9FFF, 0x3400, 0x4DBF, 0x20000, 0x2A6DF, 0x2A700, 0x2B73F, 0x2B740, 0x2B81F, 0x2B920, 0x2CEAF,
                                0xF900, 0xFAFF, 0x2F800, 0x2FA1F)]
            + list("«»·‐—…‹›"))
LETTERS = list("abcdeé") + ["ж", "か", "한"]


def random_text(rng):
    out = []
    for _ in range(rng.randint(0, 40)):
        r = rng.random()
        if r < 0.45:
            out.append("".join(rng.choice(LETTERS) for _ in range(rng.randint(1, 6))))
        elif r < 0.65:
            out.append(" ")
        else:
            out.append(rng.choice(ALPHABET))
    return "".join(out)


def make_split():
    norm = normalizers.BertNormalizer(clean_text=False, handle_chinese_chars=True, strip_accents=False, lowercase=False)
    pre = pre_tokenizers.BertPreTokenizer()
    return lambda text: [w for w, _ in pre.pre_tokenize_str(norm.normalize_str(text))]


def main():
    rng = random.Random(20261021)
    split = make_split()
    cases = [{"text": t, "words": split(t)} for t in (random_text(rng) for _ in range(300))]
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "count_tokenizers_cases.json")
    with open(path, "w") as f:
        json.dump({"tokenizers": tokenizers.__version__, "cases": cases}, f, ensure_ascii=True, indent=0)


if __name__ == "__main__":
    main()
