"""The quality model (tests/quality_model.py) held against independent forms: the words of a row against
count_model.split on valid text, the lines against bytes.split, the characters against a local restatement of the
decoder's rule, the classes against unicodedata, the duplicate lines against a set loop; every rule at equality (passes),
one past it (fails) and with a zero denominator."""
import random
import unicodedata

import count_model as CM
import offsets_model as OM
import quality_model as Q

S = Q.S
PIECES = ["a", "B", "c", "é", "Ж", "中", "\U0001F600", "-", ",", ".", "...", "…", "•", "#", " ", "\t", "▁", "\n", "\n\n", "7", "٣", "the", "of", "x" * 40]
BAD = [b"\xff", b"\xc3", b"\xe4\xb8", b"\x80", b"\xf0\x9f", b"\xe2\x80", b"\xc0\xaf", b"\xed\xa0\x80"]


def random_row(rng, valid=False, n=30):
    parts = []
    for _ in range(rng.randint(0, n)):
        if not valid and rng.random() < 0.08:
            parts.append(rng.choice(BAD))
        else:
            parts.append(rng.choice(PIECES).encode())
    return b"".join(parts)


def local_characters(row):
    """the rule as the header words it: a lead byte starts a character iff its sequence lies inside the row and is valid;
    every byte no such sequence covers is a character of its own"""
    n = len(row)
    length = [0] * n
    for p in range(n):
        cps, starts = OM.decode_with_starts(row[p:p + 4])
        if starts and starts[0] == 0:
            length[p] = OM.seq_len(row[p])
    out = []
    for p in range(n):
        if length[p]:
            out.append((p, length[p]))
        elif not any(p - d >= 0 and length[p - d] > d for d in (1, 2, 3)):
            out.append((p, 1))
    return out


def test_characters_are_the_decoders_and_one_per_dropped_byte():
    rng = random.Random(1)
    for _ in range(400):
        row = random_row(rng)
        chars = Q.characters(row)
        assert [(s, n) for s, n, _ in chars] == local_characters(row), row
        cps, starts = OM.decode_with_starts(row)
        assert [(s, c) for s, _, c in chars if c is not None] == list(zip(starts, cps))
        covered = sum(n for _, n, c in chars if c is not None)
        assert covered + sum(1 for c in chars if c[2] is None) == len(row)


def test_words_are_the_word_counts_words_on_valid_text():
    rng = random.Random(2)
    for _ in range(400):
        row = random_row(rng, valid=True)
        chars = Q.characters(row)
        words = [row[w[0][0]:w[-1][0] + w[-1][1]] for w in Q.words_of(chars)]
        assert words == CM.split(row), row
        sig = Q.signals_of_row(row)
        assert sig[S["words"]] == len(words)
        # a word whose first character is no punctuation is a word with any character that is none
        with_text = [w for w in Q.words_of(chars) if any(not Q.is_punct(c[2]) for c in w)]
        assert sig[S["text_words"]] == len(with_text) and sig[S["text_word_chars"]] == sum(len(w) for w in with_text)


def test_lines_first_and_last_characters_begin_and_end_words():
    rng = random.Random(3)
    for _ in range(400):
        row = random_row(rng)
        lines = Q.lines_of(row)
        assert [row[b:e] for b, e in lines] == [x for x in row.split(b"\n") if x]
        assert Q.signals_of_row(row)[S["newlines"]] == row.count(b"\n")
        chars = Q.characters(row)
        words = Q.words_of(chars)
        begins = {w[0][0] for w in words}
        ends = {w[-1][0] + w[-1][1] for w in words}
        for b, e in lines:
            solid = [c for c in chars if b <= c[0] < e and not Q.is_space(c[2])]
            if solid:
                assert solid[0][0] in begins and solid[-1][0] + solid[-1][1] in ends, (row, b, e)


def test_classes_are_unicodedatas():
    row = "aZ中٣7é_ ǅ".encode()
    sig = Q.signals_of_row(row)
    text = row.decode()
    assert sig[S["alpha_chars"]] == sum(unicodedata.category(c)[0] == "L" for c in text) == 5
    assert sig[S["digit_chars"]] == 2 and sig[S["upper_chars"]] == 1 and sig[S["punct_chars"]] == 1 and sig[S["space_chars"]] == 1
    assert Q.signals_of_row(b"\xff\x80a")[S["alpha_chars"]] == 1 and Q.signals_of_row(b"\xff\x80a")[S["invalid"]] == 2


def test_duplicate_lines_against_a_set_loop():
    rng = random.Random(4)
    for _ in range(300):
        row = b"\n".join(rng.choice([b"aa", b"b", b"", b"aa ", b"c\xff", b"\xe4\xb8\xad"]) for _ in range(rng.randint(0, 12)))
        seen, dup, dup_chars = set(), 0, 0
        for line in row.split(b"\n"):
            if not line:
                continue
            if line in seen:
                dup += 1
                dup_chars += len(Q.characters(line))
            seen.add(line)
        sig = Q.signals_of_row(row)
        assert (sig[S["dup_lines"]], sig[S["dup_line_chars"]]) == (dup, dup_chars)
        off = Q.signals_of_row(row, dup_lines=False)
        assert off[S["dup_lines"]] == off[S["dup_line_chars"]] == 0 and off[:21] == sig[:21]
    assert Q.signals_of_row(b"x\ny\nx")[S["dup_lines"]] == 1  # the last line without a line feed
    assert Q.signals_of_row(b"x\nx\nx\n")[S["dup_lines"]] == 2


def test_pinned_signals():
    sig = Q.signals_of_row("- The cat... sat!\n• of # …\n   \nwait...\n".encode(), stop_words=[b"the", b"of"])
    g = lambda k: sig[S[k]]
    assert (g("lines"), g("newlines"), g("bullet_lines"), g("ellipsis_lines"), g("terminal_lines"), g("short_lines")) == (4, 4, 2, 2, 2, 4)
    assert (g("ellipses"), g("hashes"), g("stop_words"), g("words"), g("text_words"), g("alpha_words")) == (3, 1, 2, 16, 5, 5)
    assert Q.signals_of_row(b"a..")[S["ellipsis_lines"]] == 0 and Q.signals_of_row(b"...")[S["ellipsis_lines"]] == 1
    assert Q.signals_of_row(b".\n..")[S["ellipses"]] == 0 and Q.signals_of_row(b"......")[S["ellipses"]] == 1
    assert Q.signals_of_row(b"x" * 30)[S["short_lines"]] == 1 and Q.signals_of_row(b"x" * 31)[S["short_lines"]] == 0
    assert Q.signals_of_row(b"x" * 31, short_line_chars=31)[S["short_lines"]] == 1


# rule -> (numerator signal, denominator signal or None, fails when "under" / "over")
RULE_FORMS = [("text_words", None, "under"), ("text_words", None, "over"), ("text_word_chars", "text_words", "under"),
              ("text_word_chars", "text_words", "over"), ("hashes", "words", "over"), ("ellipses", "words", "over"), ("bullet_lines", "lines", "over"),
              ("ellipsis_lines", "lines", "over"), ("alpha_words", "words", "under"), ("stop_words", None, "under"), ("dup_lines", "lines", "over"),
              ("dup_line_chars", "chars", "over"), ("terminal_lines", "lines", "under"), ("short_lines", "lines", "over"), ("newlines", "words", "over")]


def test_every_rule_at_equality_one_past_and_with_a_zero_denominator():
    for r, (num, den, side) in enumerate(RULE_FORMS):
        limit = [-1] * 16
        sig = [0] * 23
        if den is None:
            sig[S[num]] = 7
            limit[r] = 7
            assert Q.reasons_of(sig, limit) == 0
            sig[S[num]] += -1 if side == "under" else 1
            assert Q.reasons_of(sig, limit) == 1 << r
        else:
            sig[S[num]], sig[S[den]], limit[r] = 3, 8, 375  # 3 * 1000 == 375 * 8
            assert Q.reasons_of(sig, limit) == 0
            limit[r] += 1 if side == "under" else -1
            assert Q.reasons_of(sig, limit) == 1 << r
            sig[S[num]], sig[S[den]] = 0, 0
            for L in (0, 1, 10 ** 9):
                limit[r] = L
                assert Q.reasons_of(sig, limit) == 0
        off = [-1] * 16
        assert Q.reasons_of([5] * 23, off) == 0
    big = [2 ** 32 - 1] * 23
    # the largest signals under the largest limits (products of 62 bits): the ratio of 1000 lies under 10^6, the count over 10^9
    assert Q.reasons_of(big, [10 ** 9] * 15 + [-1]) == (1 << 1) | (1 << 2) | (1 << 8) | (1 << 12)


def test_quality_of_a_batch_keeps_the_rows_without_reasons():
    data = b"the cat\n\nof\n#"
    off = [0, 8, 8, 9, 12, 13]
    q = Q.quality(data, off, limit=Q.limits(min_text_words=1, max_hash_per_word=0), stop_words=[b"the"])
    assert q["reasons"] == [0, 1, 1, 0, 17] and q["kept"] == [0, 3] and q["data"] == b"the cat\nof\n" and q["row_off"] == [0, 8, 11]
    assert q["stats"]["rule_failed"][:5] == [3, 0, 0, 0, 1] and q["stats"]["n_kept"] == 2 and q["stats"]["n_bytes"] == 13
    assert q["signals"][S["stop_words"]] == [1, 0, 0, 0, 0]
