"""The masking contract (include/wordpiece_amd.h, section "masking") in plain Python: the classes of a cell, start,
word_ids, the counter-based draw, the masked-language-model transform and its statistics.  The GPU tests compare the
library with this bit for bit; test_mask_model.py pins it to known answers, hand-written cases and its properties.

Input: a batch ids[n_rows][max_len] and optional lengths[n_rows] (None: every column is inside; a length is clamped to
[0, max_len]); flags[x] = wp_vocab_token_flags(x) (bit0 word-initial, bit1 special, bit2 malformed), V = len(flags).
For row r, column c, x = ids[r][c]:
  outside(c): c >= len_r, or x < 0, or x >= V, or x equals one of cls_id, sep_id, pad_id that is >= 0
  solo(c):    not outside and flags[x] & 6          ([UNK] and its kin are a word of their own)
  cont(c):    not outside, not solo, not flags[x] & 1   (a "##" token)
  start(c):   not outside(c) and (not cont(c) or c == 0 or outside(c - 1) or solo(c - 1))
  word_ids[r][c]: -1 if outside, else (number of start(c') for o < c' <= c) - 1, o the last outside column before c
  w(c): the last c' <= c with start(c'); the unit u(c) is w(c) with whole_word, else c; selectable: not solo(u(c))
  selected(c): not outside(c) and selectable and draw(seed, row_base + r, u(c), 0) < select_q32
  selected: labels = x; t = draw(seed, row_base + r, c, 1); t < mask_q32: out = mask_id; else t < mask_q32 + random_q32:
    out = (draw(seed, row_base + r, c, 2) * V) >> 32; else out = x.   Not selected: out = x, labels = ignore_id.
  mix(x): x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31      (mod 2^64)
  draw(seed, row, col, stream) = mix(mix(seed + G * (row + 1)) + G * (4 * col + stream + 1)) >> 32, G = 0x9E3779B97F4A7C15
"""
from collections import namedtuple

import numpy as np

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
ONE = 1 << 32  # a q32 of "always"

Spec = namedtuple("Spec", "max_len cls_id sep_id pad_id mask_id ignore_id whole_word select_q32 mask_q32 random_q32 seed row_base")
Spec.__new__.__defaults__ = (-1, -1, -1, 0, -100, 1, 0, 0, 0, 0, 0)  # (everything behind max_len)


def q32(p):
    """a share p as the C ABI takes it"""
    return min(int(p * 4294967296.0), ONE)


def mix(x):
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def draw(seed, row, col, stream):
    return mix(mix(seed + G * (row + 1)) + G * (4 * col + stream + 1)) >> 32


def _mix_np(x):
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def draw_row(seed, row, n_cols, stream):
    """draw(seed, row, c, stream) for c in range(n_cols), as Python ints (the same arithmetic in numpy's uint64)"""
    key = mix((seed + G * (row + 1)) & M64)
    with np.errstate(over="ignore"):
        cols = np.arange(n_cols, dtype=np.uint64)
        x = np.uint64(key) + np.uint64(G) * (np.uint64(4) * cols + np.uint64(stream + 1))
        return [int(d) for d in _mix_np(x) >> np.uint64(32)]


def structure(flags, row, length, spec):
    """-> (outside, solo, start, word_ids, w) of one row, lists over its columns"""
    V, n = len(flags), len(row)
    ln = n if length is None else max(0, min(int(length), n))
    outside, solo, start, wid, w = [], [], [], [], []
    count, open_start = 0, -1
    for c, x in enumerate(row):
        x = int(x)
        o = c >= ln or x < 0 or x >= V or any(s >= 0 and x == s for s in (spec.cls_id, spec.sep_id, spec.pad_id))
        so = not o and (flags[x] & 6) != 0
        co = not o and not so and not flags[x] & 1
        st = not o and (not co or c == 0 or outside[c - 1] or solo[c - 1])
        if o:
            count = 0
        if st:
            count += 1
            open_start = c
        outside.append(o)
        solo.append(so)
        start.append(st)
        wid.append(-1 if o else count - 1)
        w.append(-1 if o else open_start)
    return outside, solo, start, wid, w


def word_ids(flags, ids, lengths, spec):
    return [structure(flags, row, None if lengths is None else lengths[r], spec)[3] for r, row in enumerate(ids)]


def mask(flags, ids, lengths, spec):
    """-> dict: input_ids, labels, word_ids (lists of rows), selected (lists of bools) and stats (wp_mask_stats)"""
    V = len(flags)
    out_rows, label_rows, wid_rows, sel_rows = [], [], [], []
    st = dict(n_rows=len(ids), n_words=0, n_selected=0, n_selected_units=0, n_masked=0, n_random=0, n_kept=0,
              whole_word=spec.whole_word)
    for r, row in enumerate(ids):
        n = len(row)
        outside, solo, start, wid, w = structure(flags, row, None if lengths is None else lengths[r], spec)
        rr = (spec.row_base + r) & M64
        d0, d1, d2 = (draw_row(spec.seed, rr, n, s) for s in range(3))
        out, labels, sel = [], [], []
        for c, x in enumerate(row):
            x = int(x)
            u = w[c] if spec.whole_word else c
            chosen = not outside[c] and not solo[u] and d0[u] < spec.select_q32
            y, lab = x, spec.ignore_id
            if chosen:
                lab = x
                st["n_selected"] += 1
                st["n_selected_units"] += u == c
                if d1[c] < spec.mask_q32:
                    y = spec.mask_id
                    st["n_masked"] += 1
                elif d1[c] < spec.mask_q32 + spec.random_q32:
                    y = (d2[c] * V) >> 32
                    st["n_random"] += 1
                else:
                    st["n_kept"] += 1
            out.append(y)
            labels.append(lab)
            sel.append(chosen)
        st["n_words"] += sum(start)
        out_rows.append(out)
        label_rows.append(labels)
        wid_rows.append(wid)
        sel_rows.append(sel)
    return dict(input_ids=out_rows, labels=label_rows, word_ids=wid_rows, selected=sel_rows, stats=st)


def flags_of(lines):
    """wp_vocab_token_flags for a vocabulary of plain ASCII lines, as utils.cpp:81-121 classifies them: [..] special,
    "##" continuation, punctuation-only words of more than one character malformed"""
    punct = set("!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~ \t\n\r\v\f")
    out = []
    for t in lines:
        prefix = not t.startswith("##")
        word = t if prefix else t[2:]
        special = prefix and len(t) > 2 and t[0] == "[" and t[-1] == "]"
        malformed = len(word) > 1 and all(ch in punct for ch in word)
        out.append((1 if prefix else 0) | (2 if special else 0) | (4 if malformed else 0))
    return out
