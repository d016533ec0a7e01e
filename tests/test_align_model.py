"""tests/align_model.py against a literal transcription of the Hugging Face course's loops on seeded batches of
tests/inputs_model.py, against a recorded fixture of the `tokenizers` package's char_to_token (everywhere) and the package
itself (where it is installed), and the label rule across the windows of a sample.  No GPU."""
import json
import os
import random

import pytest

import align_model as A
import inputs_model as I
import rows_model as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "align_tokenizers_cases.json")
LETTERS = "abcdef"
VOCAB = ["[UNK]", "[CLS]", "[SEP]", "[PAD]"] + list(LETTERS) + ["##" + ch for ch in LETTERS] + ["ab", "##cd", "é", "##é", "中", ".", ","]
CLS, SEP, PAD = 1, 2, 3


def random_docs(rng, n, long=False):
    def word():
        r = rng.random()
        if r < 0.08:
            return rng.choice(("é", "aé", "中", ".", ",", "zz"))
        return "".join(rng.choice(LETTERS) for _ in range(rng.choice((1, 1, 2, 3, 5))))
    return [rng.choice((" ", "  ")).join(word() for _ in range(rng.choice((0, 1, 3, 8, 20, 45) if long else (0, 1, 3, 8)))) for _ in range(n)]


def random_spans(rng, length, n=None):
    """sorted, disjoint, non-empty spans inside [0, length + 3)"""
    n = rng.choice((0, 1, 1, 2, 3, 6)) if n is None else n
    cuts = sorted(rng.sample(range(length + 4), min(2 * n, length + 4) // 2 * 2))
    return [(cuts[i], cuts[i + 1], rng.randint(1, 9)) for i in range(0, len(cuts), 2)]


def unit_len(doc, unit):
    return len(doc.encode("utf8")) if unit == "byte" else len(doc)


def batches(seed=31):
    """(spec of the inputs call, unit, side, batch, docs): single sequences and pairs, only_first / only_second, strides
    0, 1 and W - 1, no windows, both units"""
    rng = random.Random(seed)
    model = R.Model(VOCAB)
    out = []
    for unit in ("byte", "char"):
        for pairs, trunc, side in ((0, I.ONLY_FIRST, 0), (1, I.ONLY_SECOND, 1), (1, I.ONLY_FIRST, 0), (1, I.LONGEST_FIRST, 1),
                                   (0, I.LONGEST_FIRST, 0)):
            max_len = rng.choice((12, 16, 23))
            base = I.Spec(max_len, CLS, SEP, PAD, pairs, trunc, -1)
            strides = (-1,) if trunc == I.LONGEST_FIRST else (0, 1, "W-1", -1)
            for stride in strides:
                docs = random_docs(rng, 2 * 12 if pairs else 12, long=True)
                if stride == "W-1":  # the largest stride the spec allows: budget - kF - 1 with kF as large as it gets
                    stride = (I.budget(base) - 1) // 2 if pairs else I.budget(base) - 1
                spec = base._replace(stride=stride)
                out.append((spec, unit, side, I.build(model, docs, spec, unit), docs))
    return out


def hf_sequence_ids(batch, r):
    """Encoding.sequence_ids(): None for specials and padding, else the sequence of the cell"""
    return [None if c >= batch["lengths"][r] or tuple(batch["offsets"][r][c]) == (0, 0) else batch["token_type_ids"][r][c]
            for c in range(len(batch["input_ids"][r]))]


def hf_course_positions(batch, answers, side):
    """preprocess_training_examples of the course (chapter 7, question answering), loop for loop; answers[s] = (start_char,
    end_char) or None.  Two things the course's data never shows are spelled out: a sample without an answer and a row
    without a context cell give (0, 0)."""
    start_positions, end_positions = [], []
    for i, offset in enumerate(batch["offsets"]):
        sample_idx = batch["sample"][i]
        sequence_ids = hf_sequence_ids(batch, i)
        if answers[sample_idx] is None or side not in sequence_ids:
            start_positions.append(0)
            end_positions.append(0)
            continue
        start_char, end_char = answers[sample_idx]
        idx = 0
        while sequence_ids[idx] != side:
            idx += 1
        context_start = idx
        while idx < len(sequence_ids) and sequence_ids[idx] == side:
            idx += 1
        context_end = idx - 1
        if offset[context_start][0] > start_char or offset[context_end][1] < end_char:
            start_positions.append(0)
            end_positions.append(0)
        else:
            idx = context_start
            while idx <= context_end and offset[idx][0] <= start_char:
                idx += 1
            start_positions.append(idx - 1)
            idx = context_end
            while idx >= context_start and offset[idx][1] >= end_char:
                idx -= 1
            end_positions.append(idx + 1)
    return start_positions, end_positions


def overlap_labels(batch, per_sample, side, spec):
    """the cell rule said the other way round: the first span of the sample, in order, that overlaps the token"""
    labels, index = [], []
    base = [0]
    for s in per_sample:
        base.append(base[-1] + len(s))
    for r, row in enumerate(batch["offsets"]):
        seq, s = hf_sequence_ids(batch, r), batch["sample"][r]
        row_l, row_i = [], []
        for c, (b, e) in enumerate(row):
            if seq[c] != side:
                row_l.append(spec.ignore_id)
                row_i.append(-1)
                continue
            hit = [k for k, (sb, se, _) in enumerate(per_sample[s]) if sb < e and se > b]
            if not hit:
                row_l.append(spec.outside_label)
                row_i.append(-1)
            else:
                sb, _, lab = per_sample[s][hit[0]]
                row_l.append(lab + (spec.inside_add if b > sb else 0))
                row_i.append(base[s] + hit[0])
        labels.append(row_l)
        index.append(row_i)
    return labels, index


def context_docs(docs, pairs, side):
    return docs[side::2] if pairs else docs


def test_model_equals_the_course_loops_and_the_overlap_rule():
    rng = random.Random(32)
    n = n_answer = n_windows = 0
    for ispec, unit, side, batch, docs in batches():
        ctx = context_docs(docs, ispec.pairs, side)
        per_sample = [random_spans(rng, unit_len(d, unit)) for d in ctx]
        splits, spans, labs = A.join_spans(per_sample)
        spec = A.Spec(ispec.max_len, side, outside_label=0, inside_add=10, ignore_id=-100, no_answer=0, want=7)
        got = A.align(batch["offsets"], batch["token_type_ids"], batch["lengths"], batch["sample"], splits, spans, labs, spec)
        answers = [(s[0][0], s[0][1]) if s else None for s in per_sample]
        assert (got["start_positions"], got["end_positions"]) == hf_course_positions(batch, answers, side), (ispec, unit)
        assert (got["labels"], got["span_index"]) == overlap_labels(batch, per_sample, side, spec), (ispec, unit)
        st = got["stats"]
        assert st["n_rows"] == len(batch["lengths"]) == st["n_answer_rows"] + st["n_no_answer_rows"] and st["n_spans"] == len(spans)
        assert st["n_tokens"] == sum(x != -100 for row in got["labels"] for x in row)
        assert st["n_covered"] == sum(x >= 0 for row in got["span_index"] for x in row) >= st["n_begin"]
        # lengths NULL: the padding carries (0, 0) and is no token anyway; sample NULL where row r is sample r
        assert A.align(batch["offsets"], batch["token_type_ids"], None, batch["sample"], splits, spans, labs, spec) == got
        if batch["sample"] == list(range(len(batch["sample"]))):
            assert A.align(batch["offsets"], batch["token_type_ids"], batch["lengths"], None, splits, spans, labs, spec) == got
        # each output alone is the same output, and the statistics say what was looked up
        for want in (A.LABELS, A.SPAN_INDEX, A.POSITIONS):
            one = A.align(batch["offsets"], batch["token_type_ids"], batch["lengths"], batch["sample"], splits, spans, labs, spec._replace(want=want))
            for k in ("labels", "span_index", "start_positions", "end_positions"):
                assert one[k] == (got[k] if {"labels": 1, "span_index": 2}.get(k, 4) == want else None)
            exp = dict(st) if want != A.POSITIONS else dict(st, n_covered=0, n_begin=0)
            if want != A.POSITIONS:
                exp.update(n_answer_rows=0, n_no_answer_rows=0)
            assert one["stats"] == exp
        n += 1
        n_answer += st["n_answer_rows"]
        n_windows += batch["n_windowed"]
    assert n == 28 and n_answer > 100 and n_windows > 50


def test_labels_agree_between_the_windows_of_a_sample():
    """begin and inside labels are decided by the cell alone: a token (its offsets name it) has one label and one span in
    every window that holds it, and a window that opens inside an entity opens with an inside label"""
    rng = random.Random(33)
    n_shared = n_open_inside = 0
    for ispec, unit, side, batch, docs in batches(34):
        if ispec.stride < 0:
            continue
        ctx = context_docs(docs, ispec.pairs, side)
        per_sample = [random_spans(rng, unit_len(d, unit), n=rng.choice((1, 2, 4))) for d in ctx]
        splits, spans, labs = A.join_spans(per_sample)
        spec = A.Spec(ispec.max_len, side, outside_label=0, inside_add=100, want=3)
        got = A.align(batch["offsets"], batch["token_type_ids"], batch["lengths"], batch["sample"], splits, spans, labs, spec)
        seen = {}
        for r, row in enumerate(batch["offsets"]):
            first = True
            for c, (b, e) in enumerate(row):
                if got["labels"][r][c] == -100:
                    continue
                key = (batch["sample"][r], b, e)
                val = (got["labels"][r][c], got["span_index"][r][c])
                if key in seen:
                    assert seen[key] == val
                    n_shared += 1
                seen[key] = val
                if first and val[0] > 100:
                    n_open_inside += 1
                first = False
    assert n_shared > 500 and n_open_inside > 5


def test_gap_spans_boundaries_and_shared_cells():
    """what the contract documents rather than repairs, pinned: a span that begins in a gap has no begin cell; touching is no
    overlap; a token over two spans takes the first; cells that share a source span can put start behind end"""
    #          a   b     c  (gap)  d
    offsets = [[(0, 1), (1, 3), (3, 4), (6, 8), (0, 0)]]
    splits, spans, labs = A.join_spans([[(1, 3, 5), (5, 7, 7)]])
    got = A.align(offsets, None, None, None, splits, spans, labs, A.Spec(5, 0, 0, 1, -100, -1, 7))
    assert got["labels"] == [[0, 5, 0, 8, -100]] and got["span_index"] == [[-1, 0, -1, 1, -1]]  # span 1 begins in the gap: only an inside label
    assert (got["start_positions"], got["end_positions"]) == ([1], [1])
    splits, spans, labs = A.join_spans([[(0, 2, 5), (2, 9, 7)]])
    got = A.align(offsets, None, None, None, splits, spans, labs, A.Spec(5, 0, 0, 1, -100, -1, 7))
    assert got["labels"] == [[5, 6, 8, 8, -100]] and got["span_index"] == [[0, 0, 1, 1, -1]]  # (1, 3) overlaps both: the first
    assert (got["start_positions"], got["end_positions"]) == ([0], [1])
    # a span behind the last token, and one in the blanks between tokens: nothing covered; the answer is not held
    for sp in ((8, 11, 1), (4, 6, 1)):
        splits, spans, labs = A.join_spans([[sp]])
        got = A.align(offsets, None, None, None, splits, spans, labs, A.Spec(5, 0, 0, 1, -100, -1, 7))
        assert got["labels"] == [[0, 0, 0, 0, -100]] and got["stats"]["n_covered"] == 0
        assert got["start_positions"] == ([-1] if sp[1] > 8 else [2]) and got["end_positions"] == ([-1] if sp[1] > 8 else [3])
    # WP_OPT_NORMALIZE: three cells share the source span (0, 1) (a syllable taken apart), the answer is that character
    shared = [[(0, 0), (0, 1), (0, 1), (0, 1), (1, 2), (0, 0)]]
    splits, spans, labs = A.join_spans([[(0, 1, 1)]])
    got = A.align(shared, None, None, None, splits, spans, labs, A.Spec(6, 0, 0, 1, -100, 0, 7))
    assert (got["start_positions"], got["end_positions"]) == ([3], [1]) and got["labels"] == [[-100, 1, 1, 1, 0, -100]]
    # side 1 sees the context of a pair only; lengths cut tokens off
    types = [[0, 0, 0, 1, 1, 0]]
    got = A.align(shared, types, [4], None, splits, spans, labs, A.Spec(6, 1, 0, 1, -100, 0, 7))
    assert got["labels"] == [[-100, -100, -100, 1, -100, -100]] and (got["start_positions"], got["end_positions"]) == ([3], [3])


def test_argument_rules():
    ok = ([0, 2], [(0, 1), (1, 2)], [1, 1])
    offsets = [[(0, 1)]]
    for splits, spans, msg in (([0, 2], [(0, 1), (2, 2)], "span 1 is empty"), ([0, 2], [(3, 4), (1, 2)], "span 1 begins before span 0"),
                               ([0, 2], [(0, 3), (2, 4)], "span 1 begins before span 0"), ([1, 2], ok[1], r"span_splits .*entry 0"),
                               ([0, 3], ok[1], r"span_splits .*entry 1"), ([0, 2, 1, 2], ok[1], r"span_splits .*entry 1")):
        with pytest.raises(ValueError, match=msg):
            A.align(offsets * (len(splits) - 1), None, None, None, splits, spans, [1] * len(spans), A.Spec(1))
    # the rule holds inside a sample only
    A.align(offsets * 2, None, None, None, [0, 1, 2], [(3, 4), (1, 2)], [1, 1], A.Spec(1))
    for sample, msg in (([1], "row 0"), ([0, -1], "row 1"), (None, "row 1")):
        with pytest.raises(ValueError, match="sample of " + msg):
            A.align(offsets * (2 if sample is None else len(sample)), None, None, sample, [0, 2], ok[1], ok[2], A.Spec(1))
    for spec, types, labs, msg in ((A.Spec(0), None, ok[2], "max_len"), (A.Spec(1, 1), None, ok[2], "side 1 needs"), (A.Spec(1, 2), [[0]], ok[2], "side must"),
                                   (A.Spec(1), None, None, "without span_labels"), (A.Spec(1, want=0), None, ok[2], "no output"),
                                   (A.Spec(1, want=8), None, ok[2], "bits outside")):
        with pytest.raises(ValueError, match=msg):
            A.align(offsets, types, None, None, *ok[:2], labs, spec)
    with pytest.raises(ValueError, match="no positions"):
        A.align_rows([(0, 1)], [0, 1], *ok, A.Spec(want=4))
    for rows, msg in (([1, 1], "entry 0"), ([0, 2], "entry 1"), ([0, 1, 0, 1], "entry 1")):
        with pytest.raises(ValueError, match="row_splits .*" + msg):
            A.align_rows([(0, 1)], rows, [0] * len(rows), [], [], A.Spec())
    # the ragged form is the padded form of rows laid out one per sample
    res = A.align_rows([(0, 1), (1, 3), (0, 2)], [0, 0, 2, 3, 3], [0, 1, 2, 2, 3], [(5, 6), (2, 3), (0, 9)], [1, 2, 3], A.Spec(inside_add=10, want=3))
    assert res["labels"] == [0, 2, 0] and res["span_index"] == [-1, 1, -1]  # (the spans of rows 0 and 3 meet no cell)
    assert res["stats"] == dict(n_rows=4, n_tokens=3, n_covered=1, n_begin=1, n_spans=3, n_answer_rows=0, n_no_answer_rows=0)


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def _check_case(case):
    """the model on the recorded offsets of one text, one row without specials: where both ends of the answer fall inside
    tokens, start and end are char_to_token of its first and its last character"""
    offs = [tuple(o) for o in case["offsets"]]
    begin, end = case["answer"]
    splits, spans, labs = A.join_spans([[(begin, end, 1)]])
    got = A.align([offs], None, None, None, splits, spans, labs, A.Spec(len(offs), 0, 0, 0, -100, -1, A.POSITIONS | A.SPAN_INDEX))
    inside = case["first"] is not None and case["last"] is not None
    if inside:
        assert (got["start_positions"], got["end_positions"]) == ([case["first"]], [case["last"]]), case
        assert got["span_index"][0][case["first"]:case["last"] + 1] == [0] * (case["last"] - case["first"] + 1)
    # the cells the span covers are the tokens that hold a character of it
    chars = {c for c, (b, e) in enumerate(offs) if max(b, begin) < min(e, end)}
    assert {c for c, j in enumerate(got["span_index"][0]) if j == 0} == chars, case
    return inside


def test_model_equals_recorded_tokenizers_output():
    fx = _fixture()
    assert fx["tokenizers"] == "0.22.2" and len(fx["cases"]) == 400
    n_inside = sum(_check_case(case) for case in fx["cases"])
    assert 100 < n_inside < 400  # both kinds are there


def test_model_equals_tokenizers():
    pytest.importorskip("tokenizers")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_align", os.path.join(HERE, "golden", "make_align_tokenizers_cases.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fx = _fixture()
    assert gen.VOCAB == fx["vocab"]
    tok = gen.make_tokenizer()
    rng = random.Random(35)
    n = 0
    for case in fx["cases"]:
        assert gen.record(tok, case["text"], *case["answer"]) == case  # the library still says what was recorded
    while n < 300:  # and fresh cases, not recorded
        text = gen.random_text(rng)
        begin = rng.randrange(len(text))
        end = rng.randint(begin + 1, len(text))
        if not tok.encode(text, add_special_tokens=False).ids:
            continue
        _check_case(gen.record(tok, text, begin, end))
        n += 1
