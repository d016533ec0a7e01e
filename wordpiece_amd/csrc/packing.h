// packing.h — encoded documents packed into fixed-length rows on the device (wp_pack_sequences); the contract is the
// section "pack" of include/wordpiece_amd.h, its Python statement tests/pack_model.py.  ("pack" alone names the padded
// call's pack_rows_kernel in this code base; the kernels here are seqpack_*.)
//
// A document gives pieces, a piece (document, first id, ids) gives a unit [bos] ids [eos]; P[k] is the number of cells
// of the units in front of piece k, P[n_p] = N.  The rows are ranges of that stream of N cells: in stream mode row r is
// [r L, (r + 1) L); in next-fit mode row j is [P[k_j], P[k_{j+1}]), k_0 = 0, k_{j+1} = next(k_j), where next(k) is the
// largest k' with P[k'] <= P[k] + L: a search in P, and next(k) > k because no unit is longer than L.
//
//   plan    seqpack_plan_kernel: one thread per document, its piece count and its cells, the 64-bit totals of the call;
//           two device_exclusive_scan give every document's first piece and first cell
//   pieces  seqpack_pieces_kernel: one thread per piece, its document by a search in the piece bases: P and src0 (where
//           the piece's first id lies in ids)
//   rows    next-fit only.  The row starts are the orbit of 0 under next: n_out dependent steps if walked one by one.
//           tile   seqpack_tile_kernel: a workgroup takes kPackPieceTile pieces; next(k) of each (kept in nx), then by
//                  pointer doubling in LDS, kPackLevels tables J_r[e] = the 2^r-th successor of e or "out of the tile";
//                  for EVERY piece e of the tile as a possible entry, by binary lifting through the tables: how many
//                  rows the chain from e starts inside the tile and where it leaves (the first piece behind the tile it
//                  lands on) — one 64-bit record per piece
//           spine  seqpack_spine_kernel: one lane follows the chain tile to tile, one dependent load of a record per
//                  ENTERED tile; with L > kPackPieceTile a row holds more pieces than a tile and the chain jumps over
//                  whole tiles, which keep kPackNoEntry.  Leaves per entered tile its entry piece and the row number
//                  there, and n_out
//           apply  seqpack_apply_kernel: an entered tile rebuilds the tables from nx, marks the orbit of its entry — the
//                  tables applied from the highest power down to everything marked so far, so that every hop count is
//                  produced by its binary digits — ranks the marks with a block scan and writes row_first[R + rank].
//                  No thread walks rows one by one.
//   write   seqpack_write_kernel: the flat stream of output cells in tiles of kPackCellTile, whatever the rows are (one
//           row of 10^6 cells and 10^6 rows of one cell take the same path): the rows of the tile (their first piece and
//           first stream cell) and the at most kPackCellTile + 1 entries of P its cells can fall into go to LDS — thread
//           0 narrows that range with two searches — then a lane finds the piece of each of its cells there, gathers
//           the id or takes bos / eos / pad and stores every wanted output once, coalesced.  lengths[r] comes from the
//           tile that holds the row's first cell.  The grid is capped and a workgroup takes tiles in turn: the sums of
//           lengths and of the rows' largest segment ids stay in registers, then wave reduction, LDS and two atomics
//           per workgroup (DESIGN section 13 on what one atomic per tile cost the first mask kernel).
//
// Per cell: 4 B of ids gathered, 4 B per wanted output written; per piece 20 B of tables (P, src0, nx, the record).
#pragma once
#include "common.h"
#include "primitives.h"

namespace wp {

constexpr int kPackPieceItems = 4;
constexpr int kPackPieceTile = kBlock * kPackPieceItems;  // T: pieces per tile of the rows passes
constexpr int kPackLevels = 10;                           // 2^kPackLevels == T: the chain makes at most T - 1 hops inside a tile
constexpr int kPackCellItems = 8;
constexpr int kPackCellTile = kBlock * kPackCellItems;  // C: output cells per tile of the write pass
constexpr uint32_t kPackNoEntry = 0xFFFFFFFFu;          // tile_entry of a tile the chain jumps over
constexpr uint16_t kPackOutOfTile = kPackPieceTile;     // J_r[e]: the chain has left the tile
constexpr unsigned kPackMaxGrid = 2048;                 // workgroups of the kernels that end in atomics
static_assert((1 << kPackLevels) == kPackPieceTile, "the doubling tables must cover every hop count inside a tile");

struct PackGeom {
  int max_len, budget;  // L, B = L - specials
  int stream, split;    // WP_PACK_STREAM / WP_PACK_LONG_SPLIT (next-fit only)
  int32_t bos_id, eos_id, pad_id;
  int want;
  uint32_t n_ids, n_cells, n_pieces, n_out;  // known to the host after the plan (n_out: after the spine)
};
struct PackOut {
  int32_t *input_ids, *segment_ids, *position_ids, *source, *lengths;
};

// the totals of a call, 64 bits each, in this order behind d_scalars + kScalarPack
enum PackCounter { kPackPieces = 0, kPackStream, kPackCut, kPackIdsCut, kPackEmpty, kPackRows, kPackCells, kPackSegments, kPackCounters };

// a workgroup's sums of K 64-bit values each: wave reduction, LDS, one atomic per value by thread 0
template <int K>
__device__ __forceinline__ void seqpack_add_totals(unsigned long long (&v)[K], unsigned long long (*s_sum)[K],
                                                   unsigned long long *__restrict__ totals, const int *slots) {
#pragma unroll
  for (int k = 0; k < K; k++) {
    v[k] = wave_reduce_sum64(v[k]);
    if (lane_id() == 0) s_sum[wave_id()][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 0; k < K; k++) {
      unsigned long long t = 0;
      for (int w = 0; w < kBlock / kWave; w++) t += s_sum[w][k];
      if (t) atomicAdd(&totals[slots[k]], t);
    }
  }
}

// One thread per document (grid-stride, at most kPackMaxGrid workgroups): pieces[i], cells[i] (both saturate; the host
// reads the 64-bit totals before anything relies on them) and the totals.  A descent in splits counts as length 0 (the
// check kernel beside this one reports it).
__global__ __launch_bounds__(kBlock) void seqpack_plan_kernel(const long long *__restrict__ splits, size_t n_docs, PackGeom g,
                                                              uint32_t *__restrict__ pieces, uint32_t *__restrict__ cells,
                                                              unsigned long long *__restrict__ totals) {
  __shared__ unsigned long long s_sum[kBlock / kWave][5];
  const unsigned long long s = (g.bos_id >= 0 ? 1u : 0u) + (g.eos_id >= 0 ? 1u : 0u), B = static_cast<unsigned long long>(g.budget);
  unsigned long long v[5] = {0, 0, 0, 0, 0};  // pieces, cells, documents cut, ids cut, empty documents
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n_docs; i += static_cast<size_t>(gridDim.x) * kBlock) {
    const long long a = splits[i], b = splits[i + 1];
    const unsigned long long l = b > a ? static_cast<unsigned long long>(b) - static_cast<unsigned long long>(a) : 0ull;
    unsigned long long np = 0, kept = 0;
    if (l == 0) {
      v[4]++;
    } else if (g.stream) {
      np = 1;
      kept = l;
    } else if (!g.split) {
      np = 1;
      kept = min(l, B);
      if (l > B) {
        v[2]++;
        v[3] += l - kept;
      }
    } else {
      np = (l - 1) / B + 1;
      kept = l;
    }
    const unsigned long long c = kept + np * s;
    pieces[i] = static_cast<uint32_t>(min(np, 0xFFFFFFFFull));
    cells[i] = static_cast<uint32_t>(min(c, 0xFFFFFFFFull));
    v[0] += np;
    v[1] += c;
  }
  const int slots[5] = {kPackPieces, kPackStream, kPackCut, kPackIdsCut, kPackEmpty};
  seqpack_add_totals<5>(v, s_sum, totals, slots);
}

// One thread per piece k < n_p.  piece_base, cell_base: the exclusive scans of the plan's two arrays.  P[n_p + 1],
// src0[n_p].  (All totals fit 31 bits: the host checked.)
__global__ __launch_bounds__(kBlock) void seqpack_pieces_kernel(const long long *__restrict__ splits, uint32_t n_docs,
                                                                const uint32_t *__restrict__ piece_base,
                                                                const uint32_t *__restrict__ cell_base, PackGeom g,
                                                                uint32_t *__restrict__ P, int32_t *__restrict__ src0) {
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= g.n_pieces) return;
  if (k == 0) P[g.n_pieces] = g.n_cells;
  // the document of piece k: the last i with piece_base[i] <= k (of documents with equal bases only the last has pieces)
  uint32_t lo = 0, hi = n_docs;  // the first i with piece_base[i] > k
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (piece_base[mid] <= k) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  const uint32_t i = lo - 1;  // (piece_base[0] == 0 <= k: lo >= 1)
  const uint32_t j = k - piece_base[i];  // j > 0 in split mode only: the pieces in front are full units of max_len cells
  P[k] = cell_base[i] + j * static_cast<uint32_t>(g.max_len);
  src0[k] = static_cast<int32_t>(splits[i] + static_cast<long long>(j) * g.budget);
}

// the largest k in [a, b] with P[k] <= q (P ascends; P[a] <= q is the caller's)
__device__ __forceinline__ uint32_t seqpack_last_at_or_below(const uint32_t *__restrict__ P, uint32_t a, uint32_t b, uint32_t q) {
  while (a < b) {
    const uint32_t mid = a + (b - a + 1) / 2;
    if (P[mid] <= q) {
      a = mid;
    } else {
      b = mid - 1;
    }
  }
  return a;
}

// The doubling tables of the tile that starts at piece t0 and holds n_here pieces: s_nx[e] = next(t0 + e), s_j[r][e] =
// the 2^r-th successor of e inside the tile or kPackOutOfTile.  nx_in: next() as the tile pass left it; nullptr: it is
// searched in P here (a unit has a cell at least, so next(k) <= k + L narrows the search).
__device__ __forceinline__ void seqpack_levels(const uint32_t *__restrict__ P, const uint32_t *__restrict__ nx_in, uint32_t n_p, uint32_t L,
                                               uint32_t t0, uint32_t n_here, uint32_t *s_nx, uint16_t (*s_j)[kPackPieceTile]) {
  for (uint32_t e = threadIdx.x; e < kPackPieceTile; e += kBlock) {
    uint32_t nxt = n_p;
    if (e < n_here) {
      const uint32_t k = t0 + e;
      nxt = nx_in ? nx_in[k] : seqpack_last_at_or_below(P, k + 1, n_p - k < L ? n_p : k + L, P[k] + L);  // (P[k + 1] <= P[k] + L)
    }
    s_nx[e] = nxt;
    s_j[0][e] = (e < n_here && nxt < t0 + n_here) ? static_cast<uint16_t>(nxt - t0) : kPackOutOfTile;
  }
  __syncthreads();
  for (int r = 1; r < kPackLevels; r++) {
    for (uint32_t e = threadIdx.x; e < kPackPieceTile; e += kBlock) {
      const uint16_t a = s_j[r - 1][e];
      s_j[r][e] = a == kPackOutOfTile ? kPackOutOfTile : s_j[r - 1][a];
    }
    __syncthreads();
  }
}

// Tile pass of the rows.  nx[k] = next(k); rec[k] = (the first piece behind the tile that the chain from k lands on) <<
// 32 | the rows the chain from k starts inside the tile (k's own included).  Grid: cdiv(n_p, kPackPieceTile).
__global__ __launch_bounds__(kBlock) void seqpack_tile_kernel(const uint32_t *__restrict__ P, uint32_t n_p, uint32_t L,
                                                              uint32_t *__restrict__ nx, unsigned long long *__restrict__ rec) {
  __shared__ uint32_t s_nx[kPackPieceTile];
  __shared__ uint16_t s_j[kPackLevels][kPackPieceTile];
  const uint32_t t0 = blockIdx.x * kPackPieceTile, n_here = min(static_cast<uint32_t>(kPackPieceTile), n_p - t0);
  seqpack_levels(P, nullptr, n_p, L, t0, n_here, s_nx, s_j);
  for (uint32_t e = threadIdx.x; e < n_here; e += kBlock) {
    uint32_t pos = e, rows = 1;
#pragma unroll
    for (int r = kPackLevels - 1; r >= 0; r--) {  // the last piece of the chain inside the tile, by the digits of its hop count
      const uint16_t j = s_j[r][pos];
      if (j != kPackOutOfTile) {
        pos = j;
        rows += 1u << r;
      }
    }
    nx[t0 + e] = s_nx[e];
    rec[t0 + e] = (static_cast<unsigned long long>(s_nx[pos]) << 32) | rows;
  }
}

// One lane follows the chain from piece 0 through the records: per entered tile its entry piece and the number of the
// row that starts there; row_first[n_out] = n_p; totals[kPackRows] = n_out.  tile_entry comes in as kPackNoEntry.
__global__ __launch_bounds__(kWave) void seqpack_spine_kernel(const unsigned long long *__restrict__ rec, uint32_t n_p,
                                                              uint32_t *__restrict__ tile_entry, uint32_t *__restrict__ tile_row,
                                                              uint32_t *__restrict__ row_first, unsigned long long *__restrict__ totals) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint32_t e = 0, rows = 0;
  while (e < n_p) {
    const uint32_t t = e / kPackPieceTile;
    tile_entry[t] = e;
    tile_row[t] = rows;
    const unsigned long long v = rec[e];
    rows += static_cast<uint32_t>(v);
    const uint32_t to = static_cast<uint32_t>(v >> 32);
    if (to <= e) break;  // (never: next(k) > k)
    e = to;
  }
  row_first[rows] = n_p;  // (rows <= n_p: row_first has n_p + 1 entries)
  totals[kPackRows] = rows;
}

// Apply pass of the rows: the row starts inside every entered tile.  Grid: cdiv(n_p, kPackPieceTile).
__global__ __launch_bounds__(kBlock) void seqpack_apply_kernel(const uint32_t *__restrict__ nx, uint32_t n_p, uint32_t L,
                                                               const uint32_t *__restrict__ tile_entry,
                                                               const uint32_t *__restrict__ tile_row, uint32_t *__restrict__ row_first) {
  __shared__ uint32_t s_nx[kPackPieceTile];
  __shared__ uint16_t s_j[kPackLevels][kPackPieceTile];
  __shared__ uint32_t s_mark[kPackPieceTile];
  __shared__ uint32_t s_sm[8];
  const uint32_t entry = tile_entry[blockIdx.x];
  if (entry == kPackNoEntry) return;  // the chain jumps over this tile (the whole workgroup leaves)
  const uint32_t t0 = blockIdx.x * kPackPieceTile, n_here = min(static_cast<uint32_t>(kPackPieceTile), n_p - t0);
  for (uint32_t e = threadIdx.x; e < kPackPieceTile; e += kBlock) s_mark[e] = t0 + e == entry ? 1u : 0u;
  seqpack_levels(nullptr, nx, n_p, L, t0, n_here, s_nx, s_j);
  // every piece marked so far marks its 2^r-th successor: after the rounds r = top .. 0 the pieces at every hop count
  // from the entry are marked, each by the digits of its count.  (A mark set earlier in the same round than it is read
  // gives a hop count with digit r taken twice: a piece of the same chain, marked anyway.)
  for (int r = kPackLevels - 1; r >= 0; r--) {
    for (uint32_t e = threadIdx.x; e < kPackPieceTile; e += kBlock) {
      if (s_mark[e]) {
        const uint16_t j = s_j[r][e];
        if (j != kPackOutOfTile) s_mark[j] = 1u;
      }
    }
    __syncthreads();
  }
  const uint32_t base = threadIdx.x * kPackPieceItems;
  uint32_t own = 0;
#pragma unroll
  for (int j = 0; j < kPackPieceItems; j++) own += s_mark[base + j];
  uint32_t total;
  uint32_t rank = tile_row[blockIdx.x] + block_excl_sum(own, s_sm, total);
#pragma unroll
  for (int j = 0; j < kPackPieceItems; j++) {
    if (!s_mark[base + j]) continue;
    const bool ok = rank < n_p;  // (row_first[n_p] is the spine's)
    if (wp_in_bounds(ok, kSitePack) && ok) row_first[rank] = t0 + base + j;
    rank++;
  }
}

// The write pass.  Grid: min(cdiv(n_out * L, kPackCellTile), kPackMaxGrid) workgroups, each takes tiles in turn.
// row_first: next-fit only.  o: the wanted outputs (g.want), input_ids and lengths always.
__global__ __launch_bounds__(kBlock) void seqpack_write_kernel(const int32_t *__restrict__ ids, const uint32_t *__restrict__ P,
                                                               const int32_t *__restrict__ src0, const uint32_t *__restrict__ row_first,
                                                               PackGeom g, PackOut o, unsigned long long *__restrict__ totals) {
  __shared__ uint32_t s_P[kPackCellTile + 2];     // P[k_lo ..]: the pieces the tile's cells can fall into, and one more
  __shared__ uint32_t s_rowk[kPackCellTile + 2];  // per row of the tile (and the one behind): the piece of its first cell
  __shared__ uint32_t s_rowq[kPackCellTile + 2];  // ... and where it starts in the stream
  __shared__ uint32_t s_k[2];
  __shared__ unsigned long long s_sum[kBlock / kWave][2];
  const uint32_t L = static_cast<uint32_t>(g.max_len), N = g.n_cells, n_p = g.n_pieces, total = g.n_out * L;
  const uint32_t has_bos = g.bos_id >= 0 ? 1u : 0u, has_eos = g.eos_id >= 0 ? 1u : 0u;
  const uint32_t n_tiles = (total + kPackCellTile - 1) / kPackCellTile;
  unsigned long long v[2] = {0, 0};  // sum of lengths, sum of the rows' largest segment ids
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t x0 = tile * kPackCellTile, x1 = min(x0 + kPackCellTile, total) - 1;  // the tile's first and last cell
    const uint32_t r_lo = x0 / L, r_hi = x1 / L, nr = r_hi - r_lo + 2;                  // (nr <= kPackCellTile + 1)
    __syncthreads();  // (the previous tile's LDS has been read)
    for (uint32_t i = threadIdx.x; i < nr; i += kBlock) {
      const uint32_t r = r_lo + i;  // (<= n_out)
      uint32_t k, q;
      if (g.stream) {
        q = min(r * L, N);
        k = seqpack_last_at_or_below(P, 0, n_p, q);
      } else {
        k = min(row_first[r], n_p);
        q = P[k];
      }
      s_rowk[i] = k;
      s_rowq[i] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      // the stream cells of the tile are [q_lo, q_end): padding has none
      const uint32_t q_lo = min(s_rowq[0] + (x0 - r_lo * L), s_rowq[1]);
      const uint32_t q_end = min(s_rowq[nr - 2] + (x1 - r_hi * L) + 1, s_rowq[nr - 1]);
      uint32_t k_lo = 1, k_hi = 0;
      if (q_lo < q_end) {
        k_lo = seqpack_last_at_or_below(P, s_rowk[0], s_rowk[1], q_lo);
        k_hi = seqpack_last_at_or_below(P, s_rowk[nr - 2], s_rowk[nr - 1], q_end - 1);
      }
      s_k[0] = k_lo;
      s_k[1] = k_hi;
    }
    __syncthreads();
    const uint32_t k_lo = s_k[0], k_hi = s_k[1];
    // (k_hi - k_lo + 2 <= kPackCellTile + 1 entries: every piece of the range holds a cell of the tile)
    const uint32_t n_P = k_lo <= k_hi ? min(k_hi - k_lo + 2, static_cast<uint32_t>(kPackCellTile + 2)) : 0u;
    for (uint32_t i = threadIdx.x; i < n_P; i += kBlock) s_P[i] = P[min(k_lo + i, n_p)];
    __syncthreads();
#pragma unroll 2
    for (int j = 0; j < kPackCellItems; j++) {
      const uint32_t x = x0 + j * kBlock + threadIdx.x;
      if (x > x1) continue;
      const uint32_t r = x / L, c = x - r * L, ri = r - r_lo;
      const uint32_t q0 = s_rowq[ri], len = s_rowq[ri + 1] - q0;
      int32_t id = g.pad_id, seg = 0, pos = 0, src = -1;
      if (c < len && n_P >= 2) {
        const uint32_t q = q0 + c;
        uint32_t a = 0, b = n_P - 2;  // the largest i with s_P[i] <= q
        while (a < b) {
          const uint32_t mid = (a + b + 1) >> 1;
          if (s_P[mid] <= q) {
            a = mid;
          } else {
            b = mid - 1;
          }
        }
        const uint32_t k = k_lo + a, pk = s_P[a], off = q - pk, u = s_P[a + 1] - pk;
        if (has_bos && off == 0) {
          id = g.bos_id;
        } else if (has_eos && off == u - 1) {
          id = g.eos_id;
        } else {
          const bool k_ok = k < n_p;
          const long long at = k_ok ? static_cast<long long>(src0[k]) + off - has_bos : -1;
          const bool ok = k_ok && at >= 0 && at < static_cast<long long>(g.n_ids);
          if (wp_in_bounds(ok, kSitePack) && ok) {
            src = static_cast<int32_t>(at);
            id = ids[at];
          }
        }
        seg = static_cast<int32_t>(1 + k - s_rowk[ri]);
        pos = static_cast<int32_t>(q - max(pk, q0));
      }
      const bool in = x < total;  // (x <= x1 < total: kSitePack counts only if the geometry is ever wrong)
      if (!wp_in_bounds(in, kSitePack) || !in) continue;
      o.input_ids[x] = id;
      if (g.want & 1) o.segment_ids[x] = seg;
      if (g.want & 2) o.position_ids[x] = pos;
      if (g.want & 4) o.source[x] = src;
      if (c == 0) {  // the row's first cell: its length, and its share of the statistics
        o.lengths[r] = static_cast<int32_t>(len);
        const uint32_t k_next = s_rowk[ri + 1], q_next = s_rowq[ri + 1];
        // the row's last cell lies in the piece in front of k_next unless k_next itself began in front of the row's end
        const uint32_t k_last = (g.stream ? P[min(k_next, n_p)] : q_next) == q_next ? k_next - 1 : k_next;
        v[0] += len;
        v[1] += 1 + k_last - s_rowk[ri];
      }
    }
  }
  __syncthreads();
  const int slots[2] = {kPackCells, kPackSegments};
  seqpack_add_totals<2>(v, s_sum, totals, slots);
}

}  // namespace wp
