"""The contract of the n-gram overlap search (include/wordpiece_amd.h, section "n-gram overlap") in executable form: a
dict from the bytes of a reference window to the smallest reference row that holds it, and a loop over the rows and
positions of the corpus.  Nothing here knows of keys, tiles, sorts or scans, and nothing is hashed but by Python's dict."""

WANT_MASK, WANT_REF, WANT_COMPACT = 1, 2, 4


def rows_of(data, row_off, elem_bytes):
    data = bytes(data)
    off = [int(x) for x in row_off]
    n = len(off) - 1
    assert n >= 0 and (n == 0 or off[0] == 0) and all(off[i] <= off[i + 1] for i in range(n))
    assert n == 0 or off[n] * elem_bytes <= len(data)
    return [data[off[i] * elem_bytes:off[i + 1] * elem_bytes] for i in range(n)], off


def windows(row, k, elem_bytes):
    """the windows of one row (bytes): [(p, bytes of window p)]; none where the row has fewer than k elements"""
    n = len(row) // elem_bytes
    return [(p, row[p * elem_bytes:(p + k) * elem_bytes]) for p in range(n - k + 1)]


def overlap_rows(data, row_off, ref_data, ref_off, elem_bytes=1, ngram=13, max_hits=0, want=7):
    """-> {"hits", "first_hit", "first_ref", "covered"} (lists per corpus row), "mask" (list per element), "ref_hits"
    (list per reference row), "kept" + "data" (bytes) + "row_off" on request, and "stats": the statistics the contract
    fixes."""
    assert elem_bytes in (1, 4) and 1 <= ngram <= 64 and max_hits >= 0
    rows, off = rows_of(data, row_off, elem_bytes)
    refs, roff = rows_of(ref_data, ref_off, elem_bytes)
    table = {}  # window bytes -> the smallest reference row that holds it
    n_ref_windows = 0
    for j, ref in enumerate(refs):
        for _, w in windows(ref, ngram, elem_bytes):
            table.setdefault(w, j)
            n_ref_windows += 1
    hits, first_hit, first_ref, covered, mask, seen, n_windows = [], [], [], [], [], set(), 0
    for row in rows:
        n = len(row) // elem_bytes
        cov = [0] * n
        hp = []
        for p, w in windows(row, ngram, elem_bytes):
            n_windows += 1
            if w in table:
                hp.append(p)
                seen.add(w)
                cov[p:p + ngram] = [1] * ngram
        hits.append(len(hp))
        first_hit.append(hp[0] if hp else -1)
        first_ref.append(table[row[hp[0] * elem_bytes:(hp[0] + ngram) * elem_bytes]] if hp else -1)
        covered.append(sum(cov))
        mask += cov
    res = {"hits": hits, "first_hit": first_hit, "first_ref": first_ref, "covered": covered}
    if want & WANT_MASK:
        res["mask"] = mask
    if want & WANT_REF:
        res["ref_hits"] = [sum(1 for _, w in windows(ref, ngram, elem_bytes) if w in seen) for ref in refs]
    if want & WANT_COMPACT:
        kept = [i for i in range(len(rows)) if hits[i] <= max_hits]
        res["kept"] = kept
        res["data"], res["row_off"] = join([rows[i] for i in kept], elem_bytes)
    res["stats"] = {"n_rows": len(rows), "n_ref": len(refs), "n_elems": off[-1] if rows else 0, "n_ref_elems": roff[-1] if refs else 0,
                    "n_windows": n_windows, "n_ref_windows": n_ref_windows, "n_ref_distinct": len(table), "n_hits": sum(hits),
                    "n_hit_rows": sum(1 for h in hits if h), "n_covered": sum(covered)}
    return res


def join(rows, elem_bytes=1):
    """rows (bytes each, a multiple of elem_bytes) -> (data, row_off list)"""
    off = [0]
    for row in rows:
        assert len(row) % elem_bytes == 0
        off.append(off[-1] + len(row) // elem_bytes)
    return b"".join(rows), off
