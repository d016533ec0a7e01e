"""The contract of the repeated-span search (include/wordpiece_amd.h, section "repeated spans") in executable form: a dict
from the bytes of a window to the smallest flat position that holds it, filled in one loop over the rows and positions
of the batch in order.  Nothing here knows of keys, tiles, sorts or scans, and nothing is hashed but by Python's dict."""

WANT_MASK, WANT_SRC, WANT_COMPACT, WANT_CUT = 1, 2, 4, 8


def rows_of(data, row_off, elem_bytes):
    data = bytes(data)
    off = [int(x) for x in row_off]
    n = len(off) - 1
    assert n >= 0 and (n == 0 or off[0] == 0) and all(off[i] <= off[i + 1] for i in range(n))
    assert n == 0 or off[n] * elem_bytes <= len(data)
    return [data[off[i] * elem_bytes:off[i + 1] * elem_bytes] for i in range(n)], off


def is_cont(b):
    return b & 0xc0 == 0x80


def windows(row, k, elem_bytes, utf8=False):
    """the windows of one row (bytes): [(p, bytes of window p)]; with utf8 only those that begin at a byte that is no
    continuation byte and end at the row end or in front of such a byte"""
    n = len(row) // elem_bytes
    out = []
    for p in range(n - k + 1):
        if utf8 and (is_cont(row[p]) or (p + k < n and is_cont(row[p + k]))):
            continue
        out.append((p, row[p * elem_bytes:(p + k) * elem_bytes]))
    return out


def join(rows, elem_bytes=1):
    """rows (bytes each, a multiple of elem_bytes) -> (data, row_off list)"""
    off = [0]
    for row in rows:
        assert len(row) % elem_bytes == 0
        off.append(off[-1] + len(row) // elem_bytes)
    return b"".join(rows), off


def repeat_rows(data, row_off, elem_bytes=1, ngram=50, scope=0, max_repeats=0, utf8=False, want=15):
    """-> {"repeats", "first_repeat", "first_src_row", "first_src_pos", "covered"} (lists per row), "mask" and "src" (lists
    per element), "kept" + "data" (bytes) + "row_off", "cut_data" (bytes) + "cut_off" on request, and "stats": the
    statistics the contract fixes."""
    assert elem_bytes in (1, 4) and 1 <= ngram <= 64 and scope in (0, 1) and max_repeats >= 0 and not (utf8 and elem_bytes != 1)
    rows, off = rows_of(data, row_off, elem_bytes)
    first = {}  # window bytes -> (the smallest flat position that holds it, its row)
    repeats, first_repeat, first_src_row, first_src_pos, covered, mask, src, cut, n_windows = [], [], [], [], [], [], [], [], 0
    for i, row in enumerate(rows):
        n = len(row) // elem_bytes
        cov, s, rp = [0] * n, [-1] * n, []
        for p, w in windows(row, ngram, elem_bytes, utf8):
            n_windows += 1
            at, at_row = first.setdefault(w, (off[i] + p, i))
            if at != off[i] + p and (scope == 0 or at_row < i):
                rp.append(p)
                s[p] = at
                cov[p:p + ngram] = [1] * ngram
        repeats.append(len(rp))
        first_repeat.append(rp[0] if rp else -1)
        at, at_row = first[row[rp[0] * elem_bytes:(rp[0] + ngram) * elem_bytes]] if rp else (-1, -1)
        first_src_row.append(at_row)
        first_src_pos.append(at - off[at_row] if rp else -1)
        covered.append(sum(cov))
        mask += cov
        src += s
        cut.append(b"".join(row[e * elem_bytes:(e + 1) * elem_bytes] for e in range(n) if not cov[e]))
    res = {"repeats": repeats, "first_repeat": first_repeat, "first_src_row": first_src_row, "first_src_pos": first_src_pos, "covered": covered}
    if want & WANT_MASK:
        res["mask"] = mask
    if want & WANT_SRC:
        res["src"] = src
    if want & WANT_COMPACT:
        kept = [i for i in range(len(rows)) if repeats[i] <= max_repeats]
        res["kept"] = kept
        res["data"], res["row_off"] = join([rows[i] for i in kept], elem_bytes)
    if want & WANT_CUT:
        res["cut_data"], res["cut_off"] = join(cut, elem_bytes)
    n_elems = off[-1] if rows else 0
    res["stats"] = {"n_rows": len(rows), "n_elems": n_elems, "n_windows": n_windows, "n_distinct": len(first), "n_repeats": sum(repeats),
                    "n_repeat_rows": sum(1 for r in repeats if r), "n_covered": sum(covered),
                    "n_cut_elems": n_elems - sum(covered) if want & WANT_CUT else 0}
    return res


def brute_force(data, row_off, elem_bytes=1, ngram=50, scope=0):
    """every window against every earlier one, quadratic: -> (repeats, src per element, mask per element)"""
    rows, off = rows_of(data, row_off, elem_bytes)
    flat = [(i, p, off[i] + p, w) for i, row in enumerate(rows) for p, w in windows(row, ngram, elem_bytes)]
    n_elems = off[-1] if rows else 0
    repeats, src, mask = [0] * len(rows), [-1] * n_elems, [0] * n_elems
    for j, (i, p, at, w) in enumerate(flat):
        earlier = [f for f in flat[:j] if f[3] == w]
        if earlier and (scope == 0 or earlier[0][0] < i):
            repeats[i] += 1
            src[at] = earlier[0][2]
            mask[at:at + ngram] = [1] * ngram
    return repeats, src, mask
