"""Pure-Python restatement of the model-inputs contract of include/wordpiece_amd.h (wp_linear_encode_inputs) on top of
rows_model.py: rows become samples (one row, or a pair A, B), a sample becomes one output row under a truncation
strategy or several overlapping windows.  plan() is the arithmetic alone, build() the batch."""
import collections

import rows_model as R

LONGEST_FIRST, ONLY_FIRST, ONLY_SECOND = 0, 1, 2

Spec = collections.namedtuple("Spec", "max_len cls_id sep_id pad_id pairs truncation stride")
Spec.__new__.__defaults__ = (None, None, 0, 0, LONGEST_FIRST, -1)  # (cls_id ... stride; None: no such special)


def specials(spec):
    return (spec.cls_id is not None) + (spec.sep_id is not None) * (2 if spec.pairs else 1)


def budget(spec):
    return spec.max_len - specials(spec)


def check(spec, n_rows=0):
    """The argument rules, in the library's words (ValueError)"""
    if spec.truncation not in (LONGEST_FIRST, ONLY_FIRST, ONLY_SECOND):
        raise ValueError("unknown truncation strategy")
    if spec.stride < -1:
        raise ValueError("stride must be -1 (no windows) or at least 0")
    if spec.pairs not in (0, 1):
        raise ValueError("pairs must be 0 or 1")
    if spec.max_len < 1 or budget(spec) < 0:
        raise ValueError("max_len must be at least 1 and at least the number of specials")
    if spec.truncation == LONGEST_FIRST:
        if spec.stride >= 0:
            raise ValueError("windows (stride >= 0) need the truncation only_first or only_second")
    else:
        if spec.truncation == ONLY_SECOND and not spec.pairs:
            raise ValueError("only_second needs pairs")
        if budget(spec) < max(spec.stride, 0) + 1:
            raise ValueError("max_len leaves no room for a window")
    if spec.pairs and n_rows % 2:
        raise ValueError("pairs need an even number of rows")


def plan(la, lb, spec):
    """-> (windows, cut): windows = [((a0, a1), (b0, b1)), ...], the slices of T_A and T_B in each output row of a
    sample with len(T_A) == la, len(T_B) == lb (lb == 0 without pairs); cut: the sample lost ids for good"""
    check(spec)
    B = budget(spec)
    if not spec.pairs:
        assert lb == 0
    if spec.truncation == LONGEST_FIRST:
        if la + lb <= B:
            ka, kb = la, lb
        elif la <= lb:
            ka = min(la, max(B - lb, B // 2))
            kb = min(lb, B - ka)
        else:
            kb = min(lb, max(B - la, B // 2))
            ka = min(la, B - kb)
        return [((0, ka), (0, kb))], ka < la or kb < lb
    st = max(spec.stride, 0)
    win_a = not spec.pairs or spec.truncation == ONLY_FIRST
    l, lF = (la, lb) if win_a else (lb, la)
    kF = min(lF, B - st - 1) if spec.pairs else 0
    W = B - kF
    step = W - st
    assert W >= st + 1 and step >= 1
    n_win = 1 if l <= W else 1 + -(-(l - W) // step)
    cut = kF < lF
    if spec.stride < 0:  # window 0 only
        cut = cut or n_win > 1
        n_win = 1
    wins = []
    for j in range(n_win):
        w = (j * step, min(l, j * step + W))
        wins.append((w, (0, kF)) if win_a else ((0, kF), w))
    return wins, cut


def build(model, docs, spec, unit=None):
    """The batch of `docs` (the rows: with pairs A0, B0, A1, B1, ...) -> dict: input_ids, token_type_ids (lists of
    rows), lengths, sample, offsets (rows of (begin, end), or None), n_samples, n_cut, n_windowed"""
    check(spec, len(docs))
    ids, splits, offs = R.encode_rows(model, docs, unit)
    return build_from_rows(ids, splits, offs, spec)


def build_from_rows(ids, splits, offs, spec):
    """The same from a rows result (ids, row_splits, offsets or None), whoever made it"""
    n_rows = len(splits) - 1
    check(spec, n_rows)
    k = 2 if spec.pairs else 1
    out = dict(input_ids=[], token_type_ids=[], lengths=[], sample=[], offsets=None if offs is None else [], n_samples=n_rows // k,
               n_cut=0, n_windowed=0)
    head = [] if spec.cls_id is None else [spec.cls_id]
    sep = [] if spec.sep_id is None else [spec.sep_id]
    for s in range(n_rows // k):
        a0, a1 = splits[k * s], splits[k * s + 1]
        b1 = splits[k * s + 2] if spec.pairs else a1
        wins, cut = plan(a1 - a0, b1 - a1, spec)
        out["n_cut"] += cut
        out["n_windowed"] += len(wins) > 1
        for (wa0, wa1), (wb0, wb1) in wins:
            ia, ib = range(a0 + wa0, a0 + wa1), range(a1 + wb0, a1 + wb1)
            src = [None] * len(head) + list(ia) + [None] * len(sep)
            types = [0] * len(src)
            if spec.pairs:
                src += list(ib) + [None] * len(sep)
                types += [1] * (len(ib) + len(sep))
            n = len(src)
            assert n <= spec.max_len
            row = head + [ids[i] for i in ia] + sep + ([ids[i] for i in ib] + sep if spec.pairs else [])
            out["input_ids"].append(row + [spec.pad_id] * (spec.max_len - n))
            out["token_type_ids"].append(types + [0] * (spec.max_len - n))
            out["lengths"].append(n)
            out["sample"].append(s)
            if offs is not None:
                out["offsets"].append([(0, 0) if i is None else tuple(offs[i]) for i in src] + [(0, 0)] * (spec.max_len - n))
    return out
