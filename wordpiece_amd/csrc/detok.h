// detok.h — ids back to text on the device (wp_detokenize); the contract is the section "detokenize" of
// include/wordpiece_amd.h.  ("decode" names the UTF-8 stage in this code base, decode.h; this is the way back from ids.)
//
// The text of a row is a plain concatenation of per-id byte strings: every id has two forms, form0 for the first kept
// cell of a row and form1 for a later one, both made on the host (detok_piece_bytes: the "##" rule and the clean-up
// chain of tokenizers.decoders.WordPiece) and kept in one table per context: an 8-byte record (offset, length) per
// (cleanup, form, id) and a pool of bytes beside them.  BOTH cleanup values are in the table (records of equal strings
// share their bytes), so calls that alternate between them reuse it; nothing is rebuilt.
//
// The kernels work on the flat stream of cells in tiles of kDetokTile slots, whatever the rows are: one row of 10^8
// ids and 10^6 rows of 128 cost the same.  Slot i < n_cells is cell i (ragged: ids[i]; padded: ids[i / max_len][i %
// max_len], live when the column lies below the row's length); slot n_cells is the end slot, which holds no cell and
// exists so that the rows that end there (the last one, and empty ones in front of it) have a slot to end in: a call
// has n_cells / kDetokTile + 1 tiles.  The stream of slot i is: one terminator byte for every row that ends at i, then
// the piece of cell i if it is kept.
//
//   count   detok_tile_kernel<false>: per tile the bytes of its pieces, taking "a kept cell of the same row precedes the
//           tile" for granted, and what the spine needs to put that right: len(form0) - len(form1) of the tile's
//           first kept cell if no row starts in front of it, whether a row starts in the tile, and whether a kept cell
//           follows its last row start (without a start: whether it holds a kept cell at all).
//   spine   detok_spine_kernel: one workgroup; resolves the carries through tiles that hold neither a start nor a kept
//           cell, adds the delta where the carry-in is false, scans in 64 bits, sums the statistics.
//   write   detok_tile_kernel<true>: the same tile pass with the carry-in known, then text_off of the rows that start
//           in the tile and the tile's bytes: a lane owns an aligned 4-byte word of the tile's byte range, finds the
//           slot of each of its bytes by a search in the tile's LDS array of end offsets, gathers from the pool and
//           stores once; only the partial first and last word of a tile's range go out as bytes, so no two tiles
//           touch the same word.  The range is taken in trips of kDetokTripWords words: a piece of any length works.
//
// Per cell: 4 B of ids read twice, one 8-byte record gather per pass (a second one for the first kept cell of a row),
// the piece's bytes gathered from the pool (L2-resident: about 1 MB for 30 k tokens) and written once.
#pragma once
#include <string>

#include "common.h"
#include "primitives.h"
#include "vocab.h"

namespace wp {

constexpr int kDetokItems = 8;
constexpr int kDetokTile = kBlock * kDetokItems;  // slots per tile
constexpr int kDetokTripWords = kBlock;           // 4-byte words per write trip of a workgroup
constexpr uint32_t kDetokNoPiece = 0xFFFFFFFFu;   // DetokRec.off of a malformed id: dropped

struct DetokRec {
  uint32_t off, len;
};

// ---- the host statement of the table --------------------------------------------------------------------------------
inline void detok_replace_all(std::string &s, const char *from, const char *to) {
  const std::string f(from), t(to);
  std::string out;
  size_t at = 0;
  for (;;) {
    const size_t hit = s.find(f, at);
    if (hit == std::string::npos) break;
    out.append(s, at, hit - at);
    out.append(t);
    at = hit + f.size();
  }
  if (at == 0) return;
  out.append(s, at, std::string::npos);
  s.swap(out);
}
// the clean-up of tokenizers.decoders.WordPiece(cleanup=True), over bytes, in its order
inline void detok_cleanup(std::string &s) {
  static const char *const chain[][2] = {{" .", "."},     {" ?", "?"},         {" !", "!"},   {" ,", ","},
                                         {" ' ", "'"},    {" n't", "n't"},     {" 'm", "'m"}, {" do not", " don't"},
                                         {" 's", "'s"},   {" 've", "'ve"},     {" 're", "'re"}};
  for (const auto &r : chain) detok_replace_all(s, r[0], r[1]);
}
inline void detok_append_utf8(std::string &out, uint32_t cp) {
  if (cp < 0x80) {
    out.push_back(static_cast<char>(cp));
  } else if (cp < 0x800) {
    out.push_back(static_cast<char>(0xc0 | (cp >> 6)));
    out.push_back(static_cast<char>(0x80 | (cp & 0x3f)));
  } else if (cp < 0x10000) {
    out.push_back(static_cast<char>(0xe0 | (cp >> 12)));
    out.push_back(static_cast<char>(0x80 | ((cp >> 6) & 0x3f)));
    out.push_back(static_cast<char>(0x80 | (cp & 0x3f)));
  } else {
    out.push_back(static_cast<char>(0xf0 | (cp >> 18)));
    out.push_back(static_cast<char>(0x80 | ((cp >> 12) & 0x3f)));
    out.push_back(static_cast<char>(0x80 | ((cp >> 6) & 0x3f)));
    out.push_back(static_cast<char>(0x80 | (cp & 0x3f)));
  }
}
// form0 = C(line), form1 = C(line without its "##") for a continuation token, C(" " + line) for any other
inline std::string detok_piece_bytes(const HostToken &t, int form, int cleanup) {
  std::string s;
  if (t.is_prefix) {
    if (form == 1) s.push_back(' ');
  } else if (form == 0) {
    s.append("##");
  }
  for (uint32_t cp : t.word) detok_append_utf8(s, cp);
  if (cleanup) detok_cleanup(s);
  return s;
}

// ---- the kernels ----------------------------------------------------------------------------------------------------
struct DetokGeom {
  long long n_cells, n_rows;
  int max_len;  // 0: ragged (row_splits); >= 1: padded rows of max_len cells (lengths)
  int term;     // the terminator byte, -1: none
  int n_skip;
  int32_t skip_ids[8];
  long long vocab_size;
  unsigned long long pool_bytes;  // bytes of the pool
  unsigned long long n_bytes;     // bytes of the text (write pass)
};

// what the count pass leaves per tile
struct DetokTile {
  unsigned long long sum;  // bytes of the pieces, the first kept cell in front of any row start taken as form1
  long long delta;         // len(form0) - len(form1) of that cell (kDetokHeadKept)
  uint32_t flags;
  uint32_t n_kept, n_skipped, n_dropped;
};
constexpr uint32_t kDetokHeadKept = 1;  // a kept cell lies in front of the tile's first row start
constexpr uint32_t kDetokHasStart = 2;  // a row starts in the tile
constexpr uint32_t kDetokTailKept = 4;  // a kept cell follows the last row start (no start: the tile holds a kept cell)

// the totals of a call, 64 bits each, in this order behind d_scalars + kScalarDetok
enum DetokCounter { kDetokBytes = 0, kDetokKept, kDetokSkipped, kDetokDropped, kDetokCounters };

// the first slot of row r, for 0 <= r <= n_rows (n_rows: the end slot)
__device__ __forceinline__ long long detok_first_cell(const long long *__restrict__ row_splits, const DetokGeom &g, long long r) {
  return g.max_len > 0 ? r * g.max_len : row_splits[r];
}
// the number of r in [0, n_rows] whose first slot lies below x
__device__ inline long long detok_rows_below(const long long *__restrict__ row_splits, const DetokGeom &g, long long x) {
  if (x <= 0) return 0;
  if (g.max_len > 0) return min((x + g.max_len - 1) / g.max_len, g.n_rows + 1);
  long long lo = 0, hi = g.n_rows + 1;
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if (row_splits[mid] < x) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo;
}

// One tile of kDetokTile slots.  rec: the records of the call's cleanup value, [2][vocab_size] (form, id).
// WRITE false: tiles[blockIdx.x] is written.  WRITE true: tile_off (bytes of the pieces in front of the tile) and
// tile_carry (a kept cell of the same row precedes the tile) are read, text and text_off written.
// Grid: n_cells / kDetokTile + 1 workgroups.  ids, lengths: 4-byte aligned; row_splits, text_off: 8-byte; text: 4-byte.
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void detok_tile_kernel(const int32_t *__restrict__ ids, const long long *__restrict__ row_splits,
                                                            const int32_t *__restrict__ lengths, DetokGeom g,
                                                            const DetokRec *__restrict__ rec, const uint8_t *__restrict__ pool,
                                                            DetokTile *__restrict__ tiles,
                                                            const unsigned long long *__restrict__ tile_off,
                                                            const uint32_t *__restrict__ tile_carry, uint8_t *__restrict__ text,
                                                            long long *__restrict__ text_off) {
  __shared__ int32_t s_id[kDetokTile];                 // the id of a kept cell, -1 for any other slot
  __shared__ uint32_t s_len[kDetokTile];               // bytes of the slot's piece; WRITE, in the end: of the stream through the slot
  __shared__ uint32_t s_e[kDetokTile];                 // rows that end at the slot; WRITE, in the end: through the slot
  __shared__ uint32_t s_off[WRITE ? kDetokTile : 1];   // where the slot's piece lies in the pool
  __shared__ long long s_rows[2];
  __shared__ long long s_delta;
  __shared__ int s_head;
  __shared__ uint32_t s_sm[8];
  __shared__ int32_t s_smi[8];
  __shared__ unsigned long long s_sum[kBlock / kWave][4];
  const long long t0 = static_cast<long long>(blockIdx.x) * kDetokTile;
  for (int k = threadIdx.x; k < kDetokTile; k += kBlock) s_e[k] = 0;
  if (threadIdx.x == 0) {
    s_rows[0] = detok_rows_below(row_splits, g, t0);
    s_rows[1] = detok_rows_below(row_splits, g, t0 + kDetokTile);
    s_delta = 0;
    s_head = 0;
  }
  __syncthreads();
  const long long r_lo = s_rows[0], r_hi = s_rows[1];  // the rows (and the end) whose first slot lies in the tile
  for (long long r = max(r_lo, 1ll) + threadIdx.x; r < r_hi; r += kBlock) {  // row r - 1 ends where row r starts
    const long long rel = detok_first_cell(row_splits, g, r) - t0;
    if (rel >= 0 && rel < kDetokTile) atomicAdd(&s_e[rel], 1u);
  }
  // every cell once, coalesced: kept / skipped / dropped, and the record of its form1
  uint32_t n_kept = 0, n_skipped = 0, n_dropped = 0;
#pragma unroll 2
  for (int k = 0; k < kDetokItems; k++) {
    const int slot = k * kBlock + threadIdx.x;
    const long long i = t0 + slot;
    bool live = i < g.n_cells;
    if (live && g.max_len > 0) {
      const uint32_t r = static_cast<uint32_t>(i) / static_cast<uint32_t>(g.max_len);
      const int col = static_cast<int>(static_cast<uint32_t>(i) - r * static_cast<uint32_t>(g.max_len));
      live = col < (lengths ? max(0, min(lengths[r], g.max_len)) : g.max_len);
    }
    int32_t id = -1;
    DetokRec rc{0, 0};
    if (live) {
      const int32_t x = ids[i];
      if (x < 0 || x >= g.vocab_size) {
        n_dropped++;
      } else {
        rc = rec[g.vocab_size + x];
        bool skip = false;
        for (int q = 0; q < g.n_skip; q++) skip = skip || x == g.skip_ids[q];
        if (rc.off == kDetokNoPiece) {  // malformed
          n_dropped++;
        } else if (skip) {
          n_skipped++;
        } else {
          n_kept++;
          id = x;
        }
      }
    }
    s_id[slot] = id;
    s_len[slot] = id >= 0 ? rc.len : 0u;
    if (WRITE) s_off[slot] = rc.off;
  }
  __syncthreads();
  // a thread takes kDetokItems consecutive slots: the last row start and the last kept cell at or in front of each
  const int base = threadIdx.x * kDetokItems;
  int32_t own_start = -1, own_kept = -1;
#pragma unroll
  for (int j = 0; j < kDetokItems; j++) {
    if (s_e[base + j] != 0 || t0 + base + j == 0) own_start = base + j;
    if (s_id[base + j] >= 0) own_kept = base + j;
  }
  int32_t tot_start, tot_kept;
  int32_t cur_start = block_excl_max(own_start, s_smi, tot_start);
  int32_t cur_kept = block_excl_max(own_kept, s_smi, tot_kept);
  const bool carry_in = WRITE ? tile_carry[blockIdx.x] != 0 : true;
  unsigned long long sum = 0;
  uint32_t seg_sum = 0, e_sum = 0;
  uint32_t seg[kDetokItems], ends[kDetokItems];
#pragma unroll
  for (int j = 0; j < kDetokItems; j++) {
    const int slot = base + j;
    ends[j] = s_e[slot];
    if (ends[j] != 0 || t0 + slot == 0) cur_start = slot;
    uint32_t len = s_len[slot];
    const int32_t x = s_id[slot];
    if (x >= 0) {
      const bool head = cur_start < 0 && cur_kept < 0;  // the tile's first kept cell, in front of any row start
      const bool prev = cur_start < 0 ? (cur_kept >= 0 || carry_in) : cur_kept >= cur_start;
      if (!prev || (!WRITE && head)) {
        // (0 <= x < vocab_size was the condition of being kept: kSiteDetok counts only if the two ever disagree)
        const bool ok = static_cast<unsigned long long>(x) < static_cast<unsigned long long>(g.vocab_size);
        if (wp_in_bounds(ok, kSiteDetok) && ok) {
          const DetokRec r0 = rec[x];
          if (!prev) {
            len = r0.len;
            if (WRITE) s_off[slot] = r0.off;
          } else {
            s_delta = static_cast<long long>(r0.len) - static_cast<long long>(len);  // (one cell of the tile at most)
            s_head = 1;
          }
        }
      }
      cur_kept = slot;
    }
    sum += len;
    seg[j] = len + (g.term >= 0 ? ends[j] : 0u);
    seg_sum += seg[j];
    e_sum += ends[j];
  }
  if (!WRITE) {
    unsigned long long v[4] = {sum, n_kept, n_skipped, n_dropped};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      v[k] = wave_reduce_sum64(v[k]);
      if (lane_id() == 0) s_sum[wave_id()][k] = v[k];
    }
    __syncthreads();  // (s_head and s_delta too)
    if (threadIdx.x == 0) {
      DetokTile t{};
      for (int w = 0; w < kBlock / kWave; w++) {
        t.sum += s_sum[w][0];
        t.n_kept += static_cast<uint32_t>(s_sum[w][1]);
        t.n_skipped += static_cast<uint32_t>(s_sum[w][2]);
        t.n_dropped += static_cast<uint32_t>(s_sum[w][3]);
      }
      t.delta = s_delta;
      const bool tail_kept = tot_start < 0 ? tot_kept >= 0 : tot_kept >= tot_start;
      t.flags = (s_head ? kDetokHeadKept : 0u) | (tot_start >= 0 ? kDetokHasStart : 0u) | (tail_kept ? kDetokTailKept : 0u);
      tiles[blockIdx.x] = t;
    }
    return;
  }
  // the stream of the tile: end offsets of the slots (terminators + piece) and the rows ended, both inclusive
  uint32_t seg_total, e_total;
  uint32_t seg_at = block_excl_sum(seg_sum, s_sm, seg_total);
  uint32_t e_at = block_excl_sum(e_sum, s_sm, e_total);
  __syncthreads();  // (every thread has read its slots of s_len and s_e)
#pragma unroll
  for (int j = 0; j < kDetokItems; j++) {
    seg_at += seg[j];
    e_at += ends[j];
    s_len[base + j] = seg_at;
    s_e[base + j] = e_at;
  }
  __syncthreads();
  const unsigned long long term_on = g.term >= 0 ? 1ull : 0ull;
  const unsigned long long pieces0 = tile_off[blockIdx.x];
  // rows ended in front of the tile: the r >= 1 whose first slot lies below t0
  const unsigned long long p0 = pieces0 + term_on * static_cast<unsigned long long>(r_lo - (t0 > 0 ? 1 : 0));
  const unsigned long long p1 = min(p0 + seg_total, g.n_bytes);  // (== p0 + seg_total unless the ids changed between the passes)
  // text_off[r] = the bytes of the pieces in front of the row's first slot + r terminators
  for (long long r = r_lo + threadIdx.x; r < r_hi; r += kBlock) {
    const long long rel = detok_first_cell(row_splits, g, r) - t0;
    if (rel < 0 || rel >= kDetokTile) continue;
    const unsigned long long through = rel ? s_len[rel - 1] : 0u, ended = rel ? s_e[rel - 1] : 0u;
    text_off[r] = static_cast<long long>(pieces0 + through - term_on * ended + term_on * static_cast<unsigned long long>(r));
  }
  // the bytes [p0, p1) as aligned words; a lane owns word w in every trip
  for (unsigned long long w = (p0 >> 2) + threadIdx.x; w * 4 < p1; w += kDetokTripWords) {
    const unsigned long long b0 = w * 4, lo_b = max(b0, p0), hi_b = min(b0 + 4, p1);
    if (lo_b >= hi_b) continue;
    uint32_t word = 0;
    int slot = 0;
    bool search = true;
    for (unsigned long long p = lo_b; p < hi_b; p++) {
      const uint32_t at = static_cast<uint32_t>(p - p0);
      if (search || s_len[slot] <= at) {  // the first slot whose stream ends behind `at` (at < seg_total: there is one)
        int lo = search ? 0 : slot + 1, hi = kDetokTile - 1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s_len[mid] <= at) {
            lo = mid + 1;
          } else {
            hi = mid;
          }
        }
        slot = lo;
        search = false;
      }
      const uint32_t seg0 = slot ? s_len[slot - 1] : 0u;
      const uint32_t n_term = term_on ? s_e[slot] - (slot ? s_e[slot - 1] : 0u) : 0u;
      const uint32_t q = at - seg0;
      uint32_t byte = static_cast<uint32_t>(g.term) & 0xffu;
      if (q >= n_term) {
        const unsigned long long src = static_cast<unsigned long long>(s_off[slot]) + (q - n_term);
        const bool ok = s_id[slot] >= 0 && src < g.pool_bytes;
        byte = wp_in_bounds(ok, kSiteDetok) && ok ? pool[src] : 0u;
      }
      word |= byte << (8 * static_cast<int>(p - b0));
    }
    const bool ok = hi_b <= g.n_bytes;
    if (!wp_in_bounds(ok, kSiteDetok) || !ok) continue;
    if (hi_b - lo_b == 4) {
      *reinterpret_cast<uint32_t *>(text + b0) = word;
    } else {  // the partial first or last word of the tile's range: another tile owns the rest of it
      for (unsigned long long p = lo_b; p < hi_b; p++) text[p] = static_cast<uint8_t>(word >> (8 * static_cast<int>(p - b0)));
    }
  }
}

// One workgroup over the tile records in order: carry-in of every tile, offsets in 64 bits, the totals of the call.
// tile_off[t]: bytes of the pieces in front of tile t; tile_carry[t]: a kept cell of the row that is open at the tile's
// first slot lies in an earlier tile; totals: kDetokCounters 64-bit values.
__global__ __launch_bounds__(kBlock) void detok_spine_kernel(const DetokTile *__restrict__ tiles, size_t n_tiles,
                                                             unsigned long long *__restrict__ tile_off,
                                                             uint32_t *__restrict__ tile_carry,
                                                             unsigned long long *__restrict__ totals) {
  __shared__ uint32_t s_state[kBlock];
  __shared__ uint32_t s_wave_state[kBlock / kWave];
  __shared__ unsigned long long s_wave_sum[kBlock / kWave];
  __shared__ unsigned long long s_cnt[kBlock / kWave][3];
  const int lane = lane_id(), wv = wave_id();
  uint32_t carry = 0;  // no kept cell in front of the first tile
  unsigned long long at = 0, n_kept = 0, n_skipped = 0, n_dropped = 0;
  for (size_t b = 0; b < n_tiles; b += kBlock) {
    const size_t i = b + threadIdx.x;
    DetokTile t{};
    if (i < n_tiles) t = tiles[i];
    // what the tile leaves behind: 1 a kept cell in the open row, 0 none, 2 whatever it was given
    const uint32_t d = (t.flags & kDetokTailKept) ? 1u : (t.flags & kDetokHasStart) ? 0u : 2u;
    const unsigned long long def_bits = __ballot(d != 2u), val_bits = __ballot(d == 1u);
    const unsigned long long m = def_bits & bits_up_to(lane);
    uint32_t state = m ? static_cast<uint32_t>((val_bits >> top_bit(m)) & 1ull) : 2u;
    if (lane == kWave - 1) s_wave_state[wv] = state;
    __syncthreads();
    for (int w = wv - 1; w >= 0 && state == 2u; w--) state = s_wave_state[w];
    if (state == 2u) state = carry;
    s_state[threadIdx.x] = state;
    __syncthreads();
    const uint32_t carry_in = threadIdx.x ? s_state[threadIdx.x - 1] : carry;
    unsigned long long bytes = t.sum;
    if ((t.flags & kDetokHeadKept) && !carry_in) bytes += static_cast<unsigned long long>(t.delta);
    const unsigned long long inc = wave_incl_sum64(bytes);
    if (lane == kWave - 1) s_wave_sum[wv] = inc;
    carry = s_state[kBlock - 1];
    __syncthreads();
    unsigned long long ex = inc - bytes, tot = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; w++) {
      if (w < wv) ex += s_wave_sum[w];
      tot += s_wave_sum[w];
    }
    if (i < n_tiles) {
      tile_off[i] = at + ex;
      tile_carry[i] = carry_in;
    }
    at += tot;
    n_kept += t.n_kept;
    n_skipped += t.n_skipped;
    n_dropped += t.n_dropped;
    __syncthreads();  // (the shared arrays are written again in the next round)
  }
  unsigned long long v[3] = {n_kept, n_skipped, n_dropped};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    v[k] = wave_reduce_sum64(v[k]);
    if (lane == 0) s_cnt[wv][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    totals[kDetokBytes] = at;
    for (int k = 0; k < 3; k++) totals[kDetokKept + k] = s_cnt[0][k] + s_cnt[1][k] + s_cnt[2][k] + s_cnt[3][k];
  }
}

}  // namespace wp
