"""CPU checks of tests/count_model.py, the plain-Python statement of the word counts: hand-written cases of the word rule
 and of the table, a recorded fixture of the `tokenizers` package's BERT pre-tokenizer (everywhere) and the
package itself (where it is installed)."""
import importlib.util
import json
import os
import random
from collections import Counter

import pytest

import count_model as CM

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "count_tokenizers_cases.json")


def words(text, flags=0):
    return [w.decode("utf8") for w in CM.split(text, flags)]


def test_word_rule_on_the_class_probes():
    assert words("") == [] and words("  \n\t ") == []
    assert words("hello world") == ["hello", "world"]
    assert words("a▁b") == ["a", "b"]                      # S1: U+2581 is a space
    assert words("a\u00a0b") == ["a\u00a0b"]                    # S1: U+00A0 is none
    assert words("a\u0085b") == ["a\u0085b"]
    assert words("a#b ##c") == ["a", "#", "b", "#", "#", "c"]   # S2: '#' is punctuation
    assert words("self-made, ok.") == ["self", "-", "made", ",", "ok", "."]
    assert words("x·y«y—z") == ["x", "·", "y", "«", "y", "—", "z"]
    assert words("中文ab中") == ["中", "文", "ab", "中"]  # S3: CJK characters stand alone
    assert words("\U00020000\U0002f800z") == ["\U00020000", "\U0002f800", "z"]
    assert words("かなカ 한글") == ["かなカ", "한글"]  # S3: kana, Hangul are letters
    assert words("...") == [".", ".", "."]
    assert words("[MASK] a[SEP]") == ["[", "MASK", "]", "a", "[", "SEP", "]"]      # no special-token list plays a part
    assert words(" a") == ["a"] and words("a ") == ["a"] and words("a") == ["a"]
    assert words(b"ab\xffcd \xe4\xb8 e") == ["abcd", "e"]      # invalid UTF-8 is dropped, the word goes on
    assert words("Café cafe CAFE", 7) == ["cafe", "cafe", "cafe"]
    assert words("a\u200bb\u00a0c", 1) == ["ab", "c"]           # clean: Cf dropped, Zs -> blank


def test_table_orders_limits_and_index():
    ws = CM.split("b a b c a b dddd c")
    t = CM.table(ws)
    assert t["words"] == [b"b", b"a", b"c", b"dddd"] and t["counts"] == [3, 2, 2, 1]
    assert t["word_index"] == [0, 1, 0, 2, 1, 0, 3, 2] and t["pool"] == b"bacdddd" and t["word_off"] == [0, 1, 2, 3, 7]
    t = CM.table(ws, order="count")
    assert t["words"] == [b"b", b"a", b"c", b"dddd"] == [w for w, _ in Counter(ws).most_common()]
    t = CM.table(CM.split("d c c b b a"), order="count")
    assert t["words"] == [b"c", b"b", b"d", b"a"] and t["counts"] == [2, 2, 1, 1]   # ties by first occurrence
    t = CM.table(ws, min_count=2, terminator=10)
    assert t["words"] == [b"b", b"a", b"c"] and t["pool"] == b"b\na\nc\n" and t["word_off"] == [0, 2, 4, 6]
    assert t["word_index"] == [0, 1, 0, 2, 1, 0, -1, 2]
    assert t["stats"] == dict(n_words=8, n_distinct=3, n_long=0, n_below_min=1, n_text_bytes=None)
    t = CM.table(ws, max_word_bytes=3, min_count=0, terminator=0)
    assert t["words"] == [b"b", b"a", b"c"] and t["word_index"][6] == -1 and t["pool"] == b"b\0a\0c\0"
    assert t["stats"]["n_long"] == 1 and t["stats"]["n_below_min"] == 0 and t["stats"]["n_words"] == 8
    t = CM.table([])
    assert t["words"] == [] and t["word_off"] == [0] and t["word_index"] == []
    assert CM.count_words("é é", terminator=255)["pool"] == b"\xc3\xa9\xff"
    assert CM.count_words("A a", flags=2)["stats"]["n_text_bytes"] == 3


def test_model_equals_recorded_tokenizers_output():
    fx = json.load(open(FIXTURE))
    assert fx["tokenizers"] == "0.22.2" and len(fx["cases"]) == 300
    differ = [c["text"] for c in fx["cases"] if words(c["text"]) != c["words"]]
    assert not differ, differ[:3]
    assert sum(len(c["words"]) for c in fx["cases"]) >= 5 * len(fx["cases"])  # (no fixture of empty texts)


def test_model_equals_tokenizers():
    pytest.importorskip("tokenizers")
    spec = importlib.util.spec_from_file_location("make_count", os.path.join(HERE, "golden", "make_count_tokenizers_cases.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    split = gen.make_split()
    rng = random.Random(7)
    differ = []
    for _ in range(3000):
        text = gen.random_text(rng)
        if words(text) != split(text):
            differ.append(text)
    assert not differ, differ[:3]
