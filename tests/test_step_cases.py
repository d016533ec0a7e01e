"""CPU checks of step_cases.py: the oracle and the model prove every claim with nothing of the code under test.

S cases: from the oracle's who / rank / lcp every mark's slot and its forward and backward reach (the first boundary with
lcp < len) equal the construction's; so do the local slot, the tile, the tiles and groups the reach crosses and the length of
S; the oracle's merged per-slot arrays, taken through its rank, equal step_cases.longest_matches.  K cases: the number of
marks, of marks between the covering one and the slot, n_total, the index shifts, that no token outgrows a round-0 key (no
needed group unless the case brings one); the oracle's ids equal a greedy walk over longest_matches.  The 34 M case proves
its claim from the word counts alone.

Wall time (measured on the build container): see step_cases.py."""
import numpy as np
import pytest

import oracle_lib as O
import round0_cases as R
import step_cases as K
from test_gpu_parity import _combine

T, G = K.T, K.G


def test_constants_and_table():
    """the constants come from the headers, and every named case stands in the table of the module's docstring"""
    assert K.T == 4096 and K.G == 64 * 4096 and K.COVER_CHUNK == 8192 and K.F_SEEDS == len(K.names("F")) == 48
    doc = K.__doc__
    for name in K.names():
        parts = name.split("_")
        assert any("_".join(parts[:k]) in doc for k in range(len(parts), 1, -1)), name
    assert all(n in K.names() for n in K.EMBEDDED) and all(n in K.names() for n in K.BIG)


def greedy_ids(text, vocab, want_p, want_s, unk):
    """the greedy longest-match walk over the model's answers: a word that cannot be finished is one [UNK]"""
    t = text.decode("utf-8")
    lens = [len(K.word_of(w)) for w in vocab]
    ids, p, n = [], 0, len(t)
    while p < n:
        if t[p] == " ":
            p += 1
            continue
        e = t.find(" ", p)
        e = n if e < 0 else e
        word, q = [], p
        while q < e:
            tok = want_p[q] if q == p else want_s[q]
            if tok < 0:
                word = [unk]
                break
            word.append(tok)
            q += lens[tok]
        ids += word
        p = e
    return ids


def oracle_marks(d, vocab):
    """{line: (slot, forward run, backward run)} from the oracle's rank and lcp: the run ends at the first boundary whose
    lcp is below the line's length"""
    n, rank, lcp = d["n"], d["rank"], d["lcp"]
    out, start = {}, d["n_text"] + 1
    for i, w in enumerate(vocab):
        L = len(K.word_of(w))
        slot = int(rank[start])
        assert d["who"][slot] == i
        below = np.nonzero(lcp[slot:] < L)[0]
        end = slot + int(below[0]) + 1 if len(below) else n
        above = np.nonzero(lcp[:slot] < L)[0]
        first = int(above[-1]) + 1 if len(above) else 0
        out[i] = (slot, end - slot - 1, slot - first)
        start += L + 1
    return out


def check_model(c, d, ov):
    lens = [O.lib().wpo_vocab_token_len(ov._h, i) for i in range(ov.size)]
    rank = d["rank"][:d["n_text"]]
    want_p, want_s = K.longest_matches(c.text, c.vocab)
    if len(set(c.vocab)) == len(c.vocab):   # (the GPU file asks wp_fast_encode for the same ids; of equal lines fast takes another)
        assert np.array_equal(ov.fast_encode(c.text), d["ids"]), c.name
    got_p, got_s = _combine(d, lens, "prefix")[rank], _combine(d, lens, "suffix")[rank]
    if len(set(c.vocab)) < len(c.vocab):   # duplicate lines: which of the equal lines wins is the oracle's rule, the line's text the model's
        same = lambda got, want: [c.vocab[i] if i >= 0 else None for i in got] == [c.vocab[i] if i >= 0 else None for i in want]
        assert same(got_p, want_p) and same(got_s, want_s), c.name
        return
    assert np.array_equal(got_p, np.array(want_p, dtype=np.int32)), c.name
    assert np.array_equal(got_s, np.array(want_s, dtype=np.int32)), c.name
    if not c.low_cp:
        assert greedy_ids(c.text, c.vocab, want_p, want_s, ov.unk_id) == d["ids"].tolist(), c.name


def check_s(name):
    c = K.build(name)
    ov = O.Vocab(c.vocab)
    d = ov.encode_debug(c.text)
    cl = c.claims
    assert d["n"] == cl["n"] == len(K.s_string(c.text, c.vocab)) and d["n_text"] == c.n_text, name
    if "dup" not in name:
        got = oracle_marks(d, c.vocab)
        for line, want in c.marks.items():
            assert got[line] == want, (name, line, got[line], want)
    if "local" in cl:   # the focus mark: where it stands and what its reach crosses
        slot, fwd, bwd = got[1]
        n, end, first = d["n"], slot + 1 + fwd, slot - bwd
        tile = slot // T
        cnt_end = min((tile + 1) * T, n)
        assert (slot % T, tile, fwd, bwd, end, -(-n // T)) == (cl["local"], cl["tile"], cl["fwd"], cl["bwd"], cl["fwd_end"], cl["n_tiles"]), name
        assert int(end >= cnt_end) == cl["surv_fwd"] and int(first <= tile * T) == cl["surv_bwd"], name
        assert (end // T if end < n else -1) == cl["stop_tile"], name
        whole = (end // T if end < n else n // T) - tile - 1
        assert max(0, whole) == cl["fwd_whole_tiles"], name
        if "stop_group_delta" in cl:
            assert end // G - slot // G == cl["stop_group_delta"], name
        if "bwd_whole_tiles" in cl:
            assert tile - first // T - 1 == cl["bwd_whole_tiles"] and first % T != 0, name
        if "bwd_group_delta" in cl:
            assert slot // G - first // G == cl["bwd_group_delta"], name
    if "n_marks" in cl:
        assert len(K.eligible(c.vocab)) == cl["n_marks"] == int((d["who"] >= 0).sum()) - 1, name   # ([UNK] is a line too)
    if "full_depth" in cl:
        assert len(set(c.vocab)) < len(c.vocab), name
    check_model(c, d, ov)


def check_k(name):
    c = K.build(name)
    cl = c.claims
    words = [K.word_of(w) for w in K.eligible(c.vocab)]
    assert len(words) == cl["n_marks"] and c.n_text + 1 == cl["n_total"], name
    wide = len(set(c.text.decode("utf-8")) | set("".join(c.vocab))) > 255
    assert wide == ("wide" in name), name
    st = K.expected_step_stats(c, False, cl.get("n_needed_groups", 0))
    assert st["key_lookup"] == 1 and st["packed"] == cl.get("packed", 1) and st["n_steps"] == 4 * cl["n_marks"] + 1 + 2 * cl.get("n_needed_groups", 0), name
    if "between" in cl:
        tr = (lambda s: "".join(K.WIDE.get(ch, ch) for ch in s)) if wide else (lambda s: s)
        lo, hi = tr(cl["cover"]), tr(cl["word"])
        assert sum(1 for w in words if lo < w < hi) == cl["between"] and lo in words and hi not in words, name
        assert (" " + hi + " ") in (" " + c.text.decode("utf-8") + " "), name
        if "same_class" in cl:
            mids = [w for w in K.eligible(c.vocab) if lo < K.word_of(w) < hi]
            assert all(w.startswith("##") != bool(cl["same_class"]) for w in mids), name
    if "chain" in cl:
        tr = (lambda s: "".join(K.WIDE.get(ch, ch) for ch in s)) if wide else (lambda s: s)
        for dpt in range(1, cl["chain"] + 1):
            assert tr("hijklmn"[:dpt]) in c.vocab and "##" + tr("hijklmn"[:dpt]) in c.vocab, name
    if "end_token" in cl:
        t = c.text.decode("utf-8")
        sufs = sorted(t[i:] + "\x01" for i in range(len(t)) if t[i] != " ")
        edge = sufs[0] if cl["end_token"] == "a" else sufs[-1]
        assert edge.startswith(cl["end_token"]) and t.split(" ")[-1] == cl["last_word"], name
        if cl["end_token"] == "z":
            assert sufs[-1].startswith(max(t.split(" "))), name
    if name.startswith("K_n_"):
        assert st["bucket_shift"] == {262143: 0, 262144: 1, 262145: 1, 524289: 2}[cl["n_total"]] == st["bucket_shift_all"], name
    if "shifts_differ" in cl:
        assert (st["bucket_shift"], st["bucket_shift_all"]) == ((2, 2) if cl["n_marks"] < 16384 else (1, 2)), (name, st)
        assert cl["shifts_differ"] == int(st["bucket_shift"] != st["bucket_shift_all"]), name
        assert max(len(w) for w in c.text.decode("utf-8").split(" ")) > K.MAX_ANCHOR_GAP, name
    if not wide:   # no token outgrows a round-0 key: no needed group but those of a family the case brings
        lens = R.code_lengths(c.text, c.vocab)
        assert lens is not None, name
        fam = {t for f in c.families for t in f.tokens}
        worst = max(sum(lens[ord(ch)] for ch in K.word_of(w)) for w in K.eligible(c.vocab) if w not in fam)
        assert worst <= K.KEY_BITS - 2, (name, worst)
    if c.families:
        import refine_cases as RC
        pops = [v for v in RC.group_populations(c.text, c.vocab).values() if len(v) >= 2]
        assert len(pops) == cl["n_needed_groups"] and len(pops[0]) == c.families[0].k, name
    ov = O.Vocab(c.vocab)
    check_model(c, ov.encode_debug(c.text), ov)


@pytest.mark.parametrize("name", [n for n in K.names("S") if n not in K.BIG])
def test_step_case_slot_space(name):
    check_s(name)


@pytest.mark.parametrize("name", K.names("K"))
def test_step_case_key_space(name):
    check_k(name)


@pytest.mark.parametrize("name", K.names("F"))
def test_step_composed(name):
    c = K.build(name)
    ov = O.Vocab(c.vocab)
    check_model(c, ov.encode_debug(c.text), ov)


def test_far_group_claim_from_the_word_counts():
    """S_far_group (n = 34.4 M): no encode_debug.  The mark's slot is the number of symbols of S below "m": the blanks, the
    separators and "[UNK]"; its run is the number of words "m"; the stop lies 65 groups behind the mark's group, so the first
    trip of sl_reach_global_kernel's loop over 64 groups finds none."""
    c = K.build("S_far_group")
    cl = c.claims
    text = c.text
    f = text.count(b"m")
    assert f == K.FAR_F == text.count(b"m ") and c.vocab == ["[UNK]", "m"]
    front = sum(text.count(bytes([b])) for b in set(text) if b < ord("m")) + 1 + sum(
        sum(1 for ch in K.word_of(w) if ch < "m") + 1 for w in c.vocab)
    n = len(text) + 1 + sum(len(K.word_of(w)) + 1 for w in c.vocab)
    end = front + 1 + f
    assert (n, front // T, front % T, f, end) == (cl["n"], cl["tile"], cl["local"], cl["fwd"], cl["fwd_end"])
    assert c.marks == {1: (front, f, 0)} and end < n and cl["stop_tile"] == end // T
    g0, gs = front // G, end // G
    assert gs - g0 == cl["stop_group_delta"] and gs >= g0 + 1 + K.WAVE and gs < -(-(-(-n // T)) // K.SL_GROUP), (g0, gs)


def test_between_text_is_another_population():
    for name in ("S_fwd_64", "K_cover_64_same", "K_chain"):
        c = K.build(name)
        other = K.between_text(c)
        assert abs(len(other) - len(c.text)) > T and set(other) - set(c.text), name
