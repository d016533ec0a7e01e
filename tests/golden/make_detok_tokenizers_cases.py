"""Writes tests/golden/detok_tokenizers_cases.json: random token sequences with what tokenizers.decoders.WordPiece
(prefix "##") makes of them, clean-up on and off.  Needs the `tokenizers` package; the fixture pins its behaviour
where the package is absent (tests/test_detok_model.py)."""
import json
import os
import random

import tokenizers
from tokenizers import decoders

TOKENS = ["[UNK]", "[CLS]", "[SEP]", "[PAD]", "[MASK]", "a", "the", "dog", "##s", "##ing", "do", "not", "do not", "n't",
          "##n't", "'", "'s", "'m", "'ve", "'re", "##'re", ".", ",", "?", "!", "##.", "##,", "###", "#", "is n't", "d",
          "é", "##é", "中", "##中", "\U0001f600", "##\U0001f600", "café", "x y", "##x y", ". .", "'t",
          "##do not", "s", "m", "ve", "re", "do not do not", "' '", "##'"]


def main():
    rng = random.Random(20261018)
    on, off = decoders.WordPiece(prefix="##", cleanup=True), decoders.WordPiece(prefix="##", cleanup=False)
    cases = []
    for k in range(300):
        n = rng.choice([0, 1, 1, 2, 2, 3, 4, 5, 8, 13])
        toks = [rng.choice(TOKENS) for _ in range(n)]
        cases.append({"tokens": toks, "cleanup": on.decode(toks), "plain": off.decode(toks)})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "detok_tokenizers_cases.json")
    with open(path, "w") as f:
        json.dump({"tokenizers": tokenizers.__version__, "tokens": TOKENS, "cases": cases}, f, ensure_ascii=True, indent=0)


if __name__ == "__main__":
    main()
