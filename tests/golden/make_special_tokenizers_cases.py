"""Writes tests/golden/special_tokenizers_cases.json: seeded strings that hold special-token literals, with the ids and
character offsets a `tokenizers` BERT pipeline gives them when every "[...]" line of the vocabulary is an added special
token (BertTokenizer's behaviour, split_special_tokens=False).  Needs the `tokenizers` package; the fixture pins its
behaviour where the package is absent (tests/test_special_model.py)."""
import json
import os
import random

import tokenizers
from tokenizers import Tokenizer, models, normalizers, pre_tokenizers

VOCAB = ["[UNK]", "[CLS]", "[SEP]", "[PAD]", "[MASK]", "[MASK2]", "[a]", "foo", "bar", "##bar", "[", "]", "mask", "cls",
         "hello", "##s", "cafe", "a", "b", "##b", ".", "##a", "ab", "##oo", "f", "é", "中", "#", "-"]
SPECIALS = ["[UNK]", "[CLS]", "[SEP]", "[PAD]", "[MASK]", "[MASK2]", "[a]"]
PIECES = SPECIALS + ["[MASK", "MASK]", "[", "]", "foo", "bar", "a", "b", "ab", " ", "  ", ".", "é", "中", "#", "-", "x",
                     "[a", "a]", "\n"]


def make_tokenizer():
    tok = Tokenizer(models.WordPiece({w: i for i, w in enumerate(VOCAB)}, unk_token="[UNK]"))
    tok.normalizer = normalizers.BertNormalizer(clean_text=False, handle_chinese_chars=True, strip_accents=False,
                                                lowercase=False)
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    tok.add_special_tokens(SPECIALS)
    return tok


def random_text(rng):
    return "".join(rng.choice(PIECES) for _ in range(rng.randint(1, 12)))


def main():
    rng = random.Random(20261019)
    tok = make_tokenizer()
    cases, seen = [], set()
    fixed = ["[CLS] a", "Paris is the [MASK] of France.", "foo[MASK]bar", "[mask]", "[[MASK]]", "[MASK2", "[MASK][MASK2][a]",
             "[CLS] hello [SEP]", "é[SEP]中[PAD]", "[MASK", "[", "]", "[]", "[ MASK]", "[MASK ]", "a[a]a", "[a[a]]"]
    while len(cases) < 400:
        text = fixed[len(cases)] if len(cases) < len(fixed) else random_text(rng)
        if text in seen:
            continue
        seen.add(text)
        e = tok.encode(text, add_special_tokens=False)
        cases.append({"text": text, "ids": e.ids, "offsets": [list(o) for o in e.offsets]})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "special_tokenizers_cases.json")
    with open(path, "w") as f:
        json.dump({"tokenizers": tokenizers.__version__, "vocab": VOCAB, "specials": SPECIALS, "pieces": PIECES, "cases": cases},
                  f, ensure_ascii=True, indent=0)


if __name__ == "__main__":
    main()
