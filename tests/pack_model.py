"""The Python statement of wp_pack_sequences (include/wordpiece_amd.h, section "pack"): ragged ids in, packed rows out.
The yardstick of tests/test_pack_model.py (against independent formulations), tests/test_pack_abi.py and
tests/test_gpu_pack.py (the library against this model, exactly).

pack() is the contract in its orbit form: the pieces and their units, P the prefix sums of the unit lengths, next(k) a
search in P, the row starts the orbit of 0 under next; the cells are laid out with numpy so that the model also serves
at 10^5 documents."""
import numpy as np

NEXT_FIT, STREAM = 0, 1
LONG_TRUNCATE, LONG_SPLIT = 0, 1
WANT_SEGMENTS, WANT_POSITIONS, WANT_SOURCE = 1, 2, 4
MODES = {"next_fit": NEXT_FIT, "stream": STREAM}
LONG_DOCS = {"truncate": LONG_TRUNCATE, "split": LONG_SPLIT}


def pieces(row_splits, max_len, mode=NEXT_FIT, bos_id=-1, eos_id=-1, long_docs=LONG_TRUNCATE):
    """-> (doc, first, n, stats): piece k is ids[row_splits[doc[k]] + first[k] :][: n[k]]; stats: n_docs, n_empty, n_cut,
    n_ids_cut, n_pieces."""
    splits = np.asarray(row_splits, dtype=np.int64)
    assert splits.ndim == 1 and len(splits) >= 1 and splits[0] == 0 and np.all(np.diff(splits) >= 0)
    s = int(bos_id >= 0) + int(eos_id >= 0)
    B = int(max_len) - s
    assert max_len >= 1 and B >= 1
    lens = np.diff(splits)
    docs = np.nonzero(lens > 0)[0]
    l = lens[docs]
    stats = dict(n_docs=len(lens), n_empty=int(np.sum(lens == 0)), n_cut=0, n_ids_cut=0)
    if mode == STREAM:
        doc, first, n = docs, np.zeros(len(docs), np.int64), l
    elif long_docs == LONG_TRUNCATE:
        doc, first, n = docs, np.zeros(len(docs), np.int64), np.minimum(l, B)
        stats["n_cut"] = int(np.sum(l > B))
        stats["n_ids_cut"] = int(np.sum(l - n))
    else:
        cnt = (l + B - 1) // B
        doc = np.repeat(docs, cnt)
        j = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        first = j * B
        n = np.minimum(B, np.repeat(l, cnt) - first)
    stats["n_pieces"] = len(doc)
    return doc.astype(np.int64), first.astype(np.int64), n.astype(np.int64), stats


def prefix(u):
    P = np.zeros(len(u) + 1, dtype=np.int64)
    np.cumsum(u, out=P[1:])
    return P


def next_piece(P, k, L):
    """the first piece of the row behind one that starts at piece k: the first k' > k with P[k' + 1] - P[k] > L, else n_p"""
    return int(np.searchsorted(P, P[k] + L, side="right")) - 1


def row_starts(P, L):
    """the orbit of 0 under next_piece, and n_p behind it: row j holds the pieces [starts[j], starts[j + 1])"""
    n_p = len(P) - 1
    starts, k = [], 0
    while k < n_p:
        starts.append(k)
        k = next_piece(P, k, L)
    return np.array(starts + [n_p], dtype=np.int64)


def pack(ids, row_splits, max_len, mode=NEXT_FIT, bos_id=-1, eos_id=-1, pad_id=0, long_docs=LONG_TRUNCATE, want=7):
    """-> dict: input_ids [n_out, L], lengths [n_out], segment_ids / position_ids / source [n_out, L] (None when not
    wanted), n_out, stats (wp_pack_stats as a dict)."""
    ids = np.asarray(ids, dtype=np.int32)
    splits = np.asarray(row_splits, dtype=np.int64)
    L = int(max_len)
    doc, first, n, stats = pieces(splits, L, mode, bos_id, eos_id, long_docs)
    has_bos, has_eos = int(bos_id >= 0), int(eos_id >= 0)
    u = n + has_bos + has_eos
    P = prefix(u)
    n_p, N = len(n), int(P[-1])
    if mode == STREAM:
        n_out = (N + L - 1) // L
        row_q0 = np.minimum(np.arange(n_out + 1, dtype=np.int64) * L, N)  # where row r starts in the stream
    else:
        starts = row_starts(P, L)
        n_out = len(starts) - 1
        row_q0 = P[starts]
    out = dict(input_ids=np.full((n_out, L), pad_id, np.int32), lengths=np.diff(row_q0).astype(np.int32),
               segment_ids=np.zeros((n_out, L), np.int32) if want & WANT_SEGMENTS else None,
               position_ids=np.zeros((n_out, L), np.int32) if want & WANT_POSITIONS else None,
               source=np.full((n_out, L), -1, np.int32) if want & WANT_SOURCE else None, n_out=n_out)
    # the stream of N cells
    q = np.arange(N, dtype=np.int64)
    k = np.repeat(np.arange(n_p, dtype=np.int64), u)
    off = q - P[k]
    is_bos = (off == 0) & bool(has_bos)
    is_eos = (off == u[k] - 1) & bool(has_eos)
    src = np.where(is_bos | is_eos, -1, splits[doc[k]] + first[k] + off - has_bos)
    val = np.where(is_bos, bos_id, np.where(is_eos, eos_id, ids[np.maximum(src, 0)] if len(ids) else 0)).astype(np.int32)
    row = np.searchsorted(row_q0, q, side="right") - 1
    col = q - row_q0[row]
    row_k0 = k[row_q0[:n_out]] if N else np.zeros(0, np.int64)  # the piece of every row's first cell
    seg = 1 + k - row_k0[row]
    pos = q - np.maximum(P[k], row_q0[row])
    out["input_ids"][row, col] = val
    if want & WANT_SEGMENTS:
        out["segment_ids"][row, col] = seg
    if want & WANT_POSITIONS:
        out["position_ids"][row, col] = pos
    if want & WANT_SOURCE:
        out["source"][row, col] = src
    n_segments = 0
    if n_out:
        last = row_q0[1:] - 1  # (every row holds a cell)
        n_segments = int(np.sum(1 + k[last] - row_k0))
    stats.update(n_out=n_out, n_cells=N, n_segments=n_segments)
    out["stats"] = stats
    return out


# ---- the decompositions of csrc/packing.h, with the tile sizes as arguments ------------------------------------------
def rows_by_tiles(P, L, T):
    """row_starts(P, L) as the rows passes compute it with tiles of T pieces (T a power of two): per tile the doubling
    tables and a record per possible entry, a spine over the entered tiles, the marks of every entered tile.
    -> (starts, entered tiles, tiles)"""
    n_p = len(P) - 1
    levels = T.bit_length() - 1
    assert 1 << levels == T and n_p >= 1
    n_tiles = (n_p + T - 1) // T
    nx = [next_piece(P, k, L) for k in range(n_p)]
    OUT = T

    def tables(t):
        t0 = t * T
        n_here = min(T, n_p - t0)
        J = [[(nx[t0 + e] - t0) if e < n_here and nx[t0 + e] < t0 + n_here else OUT for e in range(T)]]
        for r in range(1, levels):
            J.append([OUT if J[r - 1][e] == OUT else J[r - 1][J[r - 1][e]] for e in range(T)])
        return t0, n_here, J

    rec = [None] * n_p
    for t in range(n_tiles):
        t0, n_here, J = tables(t)
        for e in range(n_here):
            pos, rows = e, 1
            for r in range(levels - 1, -1, -1):
                if J[r][pos] != OUT:
                    pos, rows = J[r][pos], rows + (1 << r)
            rec[t0 + e] = (nx[t0 + pos], rows)
    entry, row_at = [None] * n_tiles, [None] * n_tiles
    e = rows = 0
    while e < n_p:  # the spine: one step per entered tile
        t = e // T
        assert entry[t] is None
        entry[t], row_at[t] = e, rows
        rows += rec[e][1]
        e = rec[e][0]
    starts = [None] * rows + [n_p]
    for t in range(n_tiles):
        if entry[t] is None:
            continue  # the chain jumps over the tile
        t0, n_here, J = tables(t)
        mark = [t0 + e == entry[t] for e in range(T)]
        for r in range(levels - 1, -1, -1):
            for e in [e for e in range(T) if mark[e]]:  # (the marks as they stood in front of the round)
                if J[r][e] != OUT:
                    mark[J[r][e]] = True
        rank = row_at[t]
        for e in range(T):
            if mark[e]:
                starts[rank] = t0 + e
                rank += 1
    return np.array(starts, dtype=np.int64), sum(x is not None for x in entry), n_tiles


def _last_at_or_below(P, a, b, q):
    assert P[a] <= q
    while a < b:
        mid = a + (b - a + 1) // 2
        if P[mid] <= q:
            a = mid
        else:
            b = mid - 1
    return a


def cells_by_tiles(P, N, L, n_out, stream, starts, C):
    """The geometry of the write pass with tiles of C cells: per output cell (row-major) the piece it lies in, -1 for
    padding; per row its length, its first piece and its largest segment id.  The ranges the kernel narrows its searches
    to are asserted on the way."""
    n_p = len(P) - 1
    total = n_out * L
    piece = np.full(total, -1, dtype=np.int64)
    lengths, row_k0, row_seg = [0] * n_out, [0] * n_out, [0] * n_out
    for x0 in range(0, total, C):
        x1 = min(x0 + C, total) - 1
        r_lo, r_hi = x0 // L, x1 // L
        nr = r_hi - r_lo + 2
        assert nr <= C + 1
        rowk, rowq = [], []
        for r in range(r_lo, r_lo + nr):
            if stream:
                q = min(r * L, N)
                k = _last_at_or_below(P, 0, n_p, q)
            else:
                k = int(starts[r])
                q = int(P[k])
            rowk.append(k)
            rowq.append(q)
        q_lo = min(rowq[0] + (x0 - r_lo * L), rowq[1])
        q_end = min(rowq[nr - 2] + (x1 - r_hi * L) + 1, rowq[nr - 1])
        k_lo, k_hi = 1, 0
        if q_lo < q_end:
            k_lo = _last_at_or_below(P, rowk[0], rowk[1], q_lo)
            k_hi = _last_at_or_below(P, rowk[nr - 2], rowk[nr - 1], q_end - 1)
        n_P = k_hi - k_lo + 2 if k_lo <= k_hi else 0
        assert n_P <= C + 1
        sP = [int(P[min(k_lo + i, n_p)]) for i in range(n_P)]
        for x in range(x0, x1 + 1):
            r, c = divmod(x, L)
            ri = r - r_lo
            q0, length = rowq[ri], rowq[ri + 1] - rowq[ri]
            if c < length:
                assert n_P >= 2
                a = _last_at_or_below(sP, 0, n_P - 2, q0 + c)
                assert sP[a] <= q0 + c < sP[a + 1]
                piece[x] = k_lo + a
            if c == 0:
                k_next, q_next = rowk[ri + 1], rowq[ri + 1]
                k_last = k_next - 1 if (int(P[min(k_next, n_p)]) if stream else q_next) == q_next else k_next
                lengths[r], row_k0[r], row_seg[r] = length, rowk[ri], 1 + k_last - rowk[ri]
    return piece, lengths, row_k0, row_seg
