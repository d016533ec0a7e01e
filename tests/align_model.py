"""Pure-Python restatement of the span-alignment contract of include/wordpiece_amd.h (wp_align, wp_align_rows): the
argument rules in the library's words, the cell rule, the answer positions and the statistics, over plain lists or
numpy arrays.  Nothing here is fast; everything is literal."""
import collections

import numpy as np

LABELS, SPAN_INDEX, POSITIONS = 1, 2, 4

Spec = collections.namedtuple("Spec", "max_len side outside_label inside_add ignore_id no_answer want")
Spec.__new__.__defaults__ = (0, 0, 0, 0, -100, 0, LABELS)  # (max_len 0: the ragged form does not read it)


def check_arrays(span_splits, spans, n_rows=0, sample=None, row_splits=None, n_ids=None):
    """The array rules, first offender first, in the library's words (ValueError).  row_splits: the ragged form."""
    n_samples, n_spans = len(span_splits) - 1, len(spans)
    if row_splits is not None:
        for i in range(len(row_splits)):
            s = row_splits[i]
            if (i == 0 and s != 0) or (i + 1 < len(row_splits) and row_splits[i + 1] < s) or (i + 1 == len(row_splits) and s != n_ids):
                raise ValueError("align: row_splits must start at 0, never descend and end at n_ids (entry %d)" % i)
    for i in range(n_samples + 1):
        s = span_splits[i]
        if (i == 0 and s != 0) or (i < n_samples and span_splits[i + 1] < s) or (i == n_samples and s != n_spans):
            raise ValueError("align: span_splits must start at 0, never descend and end at n_spans (entry %d)" % i)
    for s in range(n_samples):
        for j in range(span_splits[s], span_splits[s + 1]):
            if spans[j][0] >= spans[j][1]:
                raise ValueError("align: span %d is empty (begin >= end)" % j)
            if j > span_splits[s] and spans[j - 1][1] > spans[j][0]:
                raise ValueError("align: span %d begins before span %d of its sample ends (spans must be sorted and disjoint)" % (j, j - 1))
    if row_splits is None:
        for r in range(n_rows):
            s = r if sample is None else sample[r]
            if s < 0 or s >= n_samples:
                raise ValueError("align: the sample of row %d is outside [0, n_samples)" % r)


def check_spec(spec, ragged=False, has_types=True, has_span_labels=True):
    if not ragged:
        if spec.max_len < 1:
            raise ValueError("align: max_len must be at least 1")
        if spec.side not in (0, 1):
            raise ValueError("align: side must be 0 or 1")
        if spec.side == 1 and not has_types:
            raise ValueError("align: side 1 needs token_type_ids")
    if spec.want & ~7:
        raise ValueError("align: want has bits outside 7")
    if ragged and spec.want & POSITIONS:
        raise ValueError("align: the ragged form has no positions")
    if spec.want == 0:
        raise ValueError("align: no output is wanted")
    if spec.want & LABELS and not has_span_labels:
        raise ValueError("align: labels wanted without span_labels")


def cell(b, e, span_splits, spans, span_labels, s, spec):
    """a token cell (b, e) of sample s -> (label, span_index, begin cell?)"""
    for j in range(span_splits[s], span_splits[s + 1]):  # j(c): the smallest j in J with end[j] > b
        if spans[j][1] > b:
            if spans[j][0] < e:
                begin = b <= spans[j][0]
                label = None if span_labels is None else span_labels[j] + (0 if begin else spec.inside_add)
                return label, j, begin
            break
    return spec.outside_label, -1, False


def _stats(n_rows, n_spans):
    return dict(n_rows=n_rows, n_tokens=0, n_covered=0, n_begin=0, n_spans=n_spans, n_answer_rows=0, n_no_answer_rows=0)


def align(offsets, token_type_ids, lengths, sample, span_splits, spans, span_labels, spec):
    """The padded form -> dict: labels, span_index (lists of rows), start_positions, end_positions (lists), stats; an
    output that is not wanted is None."""
    n_rows = len(offsets)
    check_spec(spec, False, token_type_ids is not None, span_labels is not None)
    check_arrays(span_splits, spans, n_rows, sample)
    st = _stats(n_rows, len(spans))
    want_cells = bool(spec.want & (LABELS | SPAN_INDEX))
    labels, index, starts, ends = [], [], [], []
    for r in range(n_rows):
        L = spec.max_len if lengths is None else max(0, min(int(lengths[r]), spec.max_len))
        s = r if sample is None else int(sample[r])
        row_l, row_i, toks = [], [], []
        for c in range(spec.max_len):
            b, e = int(offsets[r][c][0]), int(offsets[r][c][1])
            t = 0 if token_type_ids is None else int(token_type_ids[r][c])
            token = c < L and e > b and t == spec.side
            if not token:
                row_l.append(spec.ignore_id)
                row_i.append(-1)
                continue
            st["n_tokens"] += 1
            toks.append((c, b, e))
            if want_cells:
                lab, j, begin = cell(b, e, span_splits, spans, span_labels, s, spec)
                st["n_covered"] += j >= 0
                st["n_begin"] += begin
                row_l.append(lab)
                row_i.append(j)
        labels.append(row_l)
        index.append(row_i)
        if spec.want & POSITIONS:
            start = end = spec.no_answer
            held = False
            if span_splits[s + 1] > span_splits[s] and toks:
                ab, ae = int(spans[span_splits[s]][0]), int(spans[span_splits[s]][1])
                lo, hi = min(b for _, b, _ in toks), max(e for _, _, e in toks)
                if ab >= lo and ae <= hi:
                    held = True
                    start = max(c for c, b, _ in toks if b <= ab)
                    end = min(c for c, _, e in toks if e >= ae)
            st["n_answer_rows" if held else "n_no_answer_rows"] += 1
            starts.append(start)
            ends.append(end)
    return dict(labels=labels if spec.want & LABELS else None, span_index=index if spec.want & SPAN_INDEX else None,
                start_positions=starts if spec.want & POSITIONS else None, end_positions=ends if spec.want & POSITIONS else None,
                stats=st)


def align_rows(offsets, row_splits, span_splits, spans, span_labels, spec):
    """The ragged form: row i is sample i, every cell is a token -> dict: labels, span_index (flat lists), stats"""
    check_spec(spec, True, True, span_labels is not None)
    n_rows = len(row_splits) - 1
    n_ids = len(offsets)
    if len(span_splits) != n_rows + 1:
        raise ValueError("align: the ragged form needs one list of spans per row")
    check_arrays(span_splits, spans, row_splits=row_splits, n_ids=n_ids)
    st = _stats(n_rows, len(spans))
    labels, index = [], []
    for r in range(n_rows):
        for i in range(row_splits[r], row_splits[r + 1]):
            lab, j, begin = cell(int(offsets[i][0]), int(offsets[i][1]), span_splits, spans, span_labels, r, spec)
            st["n_tokens"] += 1
            st["n_covered"] += j >= 0
            st["n_begin"] += begin
            labels.append(lab)
            index.append(j)
    return dict(labels=labels if spec.want & LABELS else None, span_index=index if spec.want & SPAN_INDEX else None, stats=st)


def join_spans(per_sample):
    """[[(begin, end[, label]), ...], ...] -> (span_splits, spans, span_labels) as lists"""
    splits, spans, labs = [0], [], []
    for s in per_sample:
        for t in s:
            spans.append((t[0], t[1]))
            labs.append(t[2] if len(t) > 2 else 0)
        splits.append(len(spans))
    return splits, spans, labs


def as_arrays(res, n_rows, max_len):
    """the model's lists as the int32 arrays the library returns (None stays None)"""
    out = {}
    for k, shape in (("labels", (n_rows, max_len)), ("span_index", (n_rows, max_len)), ("start_positions", (n_rows,)),
                     ("end_positions", (n_rows,))):
        if res.get(k) is not None:
            out[k] = np.array(res[k], dtype=np.int64).astype(np.int32).reshape(shape)
    return out
