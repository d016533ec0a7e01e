// dedup.h — the kernels of the duplicate-row removal (include/wordpiece_amd.h, section "duplicate rows"; host path:
// dedup_path.h).  The input is a ragged batch: a flat element stream (1 or 4 bytes per element) and row_off.  Every row
// is cut into chunks of kDedupChunk bytes, and all work on bytes is flat over the chunk list: a chunk finds its row by
// bisection in the chunk offsets, so one row of 10^8 bytes costs what 10^6 rows of 100 do, and no lane, wave or
// workgroup walks a row.  The key of a row is the sum mod 2^64 of the seeded hashes of its chunks (each mixed with its
// index in the row) plus a mix of the length: an integer sum, whatever order the chunks arrive in.  Rows are then grouped
// as count.h groups words (stable radix sort of the keys, run heads, head positions: its kernels, as they are), every
// member is compared with the head of its run chunk by chunk, and what differs goes into the next round under another
// seed.  The sort is stable and the item list ascends, so the head of a run is its smallest row: the first occurrence.
#pragma once
#include "common.h"
#include "count.h"  // count_mix, and the head / compact kernels of a grouping round
#include "primitives.h"

namespace wp {

constexpr int kDedupChunk = 256;                    // C: bytes of a chunk (a multiple of 8)
constexpr int kDedupTile = kBlock * kDedupChunk;    // bytes a workgroup of the key and compare kernels covers
constexpr uint32_t kDedupNoBad = 0xffffffffu;       // the bad-row word while no row failed the check

// the counters of a call, 64 bits each, in d_scalars from kScalarDedup on
enum DedupCounter { kDedupEmpty = 0, kDedupCompared = 1, kDedupCounters = 4 };

// The 4 bytes [s + 4 i, s + 4 i + 4) of the data as a little-endian word, zero from byte e on.  The loads are aligned
// words that begin below e: nothing behind the word that holds byte e - 1 is touched, and what that word holds behind
// e - 1 is masked away.
__device__ __forceinline__ uint32_t dedup_word(const uint32_t *__restrict__ d32, size_t s, size_t e, uint32_t i) {
  const size_t a = s + 4u * static_cast<size_t>(i);
  const size_t wi = a >> 2;
  const uint32_t sh = static_cast<uint32_t>(a & 3u) * 8u;
  uint32_t x = d32[wi] >> sh;
  if (sh != 0 && ((wi + 1) << 2) < e) x |= d32[wi + 1] << (32u - sh);
  const size_t rem = e - a;
  if (rem < 4) x &= (1u << (8u * static_cast<uint32_t>(rem))) - 1u;
  return x;
}

// the mix of a row's length in bytes under the round's seed: what the chunk values are added to
__device__ __forceinline__ uint64_t dedup_len_mix(uint64_t seed, uint32_t len) {
  return count_mix(count_mix(seed ^ 0x9e3779b97f4a7c15ull) ^ (static_cast<uint64_t>(len) | (1ull << 40)));
}

// Row i: its offsets checked (row_off[0] == 0, no descent; the smallest bad row wins), its start in bytes, its chunks,
// and the row as item i of round 0.  Entry n_rows closes byte_off (the end of the data) and n_chunks (0) for their
// scans; the lane of that entry leaves row_off[n_rows] in *n_elems.  The arithmetic is 64-bit and clamped: offsets
// that are wild give a bad row or a size the host refuses, never an index.
__global__ __launch_bounds__(kBlock) void dedup_rows_kernel(const long long *__restrict__ row_off, size_t n_rows, uint32_t elem_bytes,
                                                            uint32_t *__restrict__ byte_off, uint32_t *__restrict__ n_chunks,
                                                            uint32_t *__restrict__ items, int32_t *__restrict__ first,
                                                            uint32_t *__restrict__ bad, unsigned long long *__restrict__ n_elems,
                                                            unsigned long long *__restrict__ counters) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  bool empty = false;
  if (i <= n_rows) {
    const long long a = row_off[i];
    const unsigned long long ab = static_cast<unsigned long long>(a) * elem_bytes;
    byte_off[i] = a < 0 || ab > 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(ab);
    if (i == n_rows) {
      n_chunks[i] = 0;
      *n_elems = static_cast<unsigned long long>(a);
    } else {
      const long long b = row_off[i + 1];
      if (b < a || (i == 0 && a != 0)) atomicMin(bad, static_cast<uint32_t>(i));
      const unsigned long long len = b < a ? 0ull : static_cast<unsigned long long>(b - a);
      const unsigned long long ch = len > 0xffffffffull ? 0xffffffffull : (len * elem_bytes + kDedupChunk - 1) / kDedupChunk;
      n_chunks[i] = static_cast<uint32_t>(ch > 0xffffffffull ? 0xffffffffull : ch);
      items[i] = static_cast<uint32_t>(i);
      first[i] = -1;
      empty = b == a;
    }
  }
  const uint32_t k = wave_reduce_sum(empty ? 1u : 0u);
  if (lane_id() == 0 && k != 0) atomicAdd(counters + kDedupEmpty, static_cast<unsigned long long>(k));
}

// cnt[j] = the chunks of item j of the next round (items[j], j < *m_dev), 0 from *m_dev on; j in [0, cap]
__global__ __launch_bounds__(kBlock) void dedup_item_chunks_kernel(const uint32_t *__restrict__ items, const uint32_t *__restrict__ m_dev, size_t cap,
                                                                   const uint32_t *__restrict__ n_chunks, size_t n_rows, uint32_t *__restrict__ cnt) {
  const size_t j = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j > cap) return;
  uint32_t k = 0;
  if (j < *m_dev && j < cap) {
    const uint32_t row = items[j];
    if (wp_in_bounds(row < n_rows, kSiteDedup)) k = n_chunks[row];
  }
  cnt[j] = k;
}

// key[j] = the mix of the length of item j: the value its chunks are added to
__global__ __launch_bounds__(kBlock) void dedup_key_init_kernel(const uint32_t *__restrict__ items, size_t m, const uint32_t *__restrict__ byte_off,
                                                                size_t n_rows, uint64_t seed, uint64_t *__restrict__ key) {
  const size_t j = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j >= m) return;
  const uint32_t row = items[j];
  uint32_t len = 0;
  if (wp_in_bounds(row < n_rows, kSiteDedup)) len = byte_off[row + 1] - byte_off[row];
  key[j] = dedup_len_mix(seed, len);
}

// the item of chunk q of the round: the last j with chunk_off[j] <= q (chunk_off: m + 1 entries, chunk_off[m] > q)
__device__ __forceinline__ uint32_t dedup_item_of(const uint32_t *__restrict__ chunk_off, size_t m, uint32_t q) {
  size_t lo = 0, hi = m;
  while (hi - lo > 1) {
    const size_t mid = (lo + hi) >> 1;
    if (chunk_off[mid] <= q) lo = mid; else hi = mid;
  }
  return static_cast<uint32_t>(lo);
}

// Chunk q of the round (mc of them, laid out item by item): the seeded hash of its at most C bytes, its index in the
// row mixed in.  The values of one item are summed inside the wave by a segmented scan (the lanes of a wave ascend in
// q, so in item) and leave it as one 64-bit atomic per wave and item segment; an item of one chunk stores its key
// without an atomic.  The number of chunks stays below 2^32: n_bytes <= UINT32_MAX and n_rows < 2^31 bound it by
// 2^24 + 2^31.
__global__ __launch_bounds__(kBlock) void dedup_keys_kernel(const uint32_t *__restrict__ d32, size_t n_bytes, const uint32_t *__restrict__ byte_off,
                                                            const uint32_t *__restrict__ items, const uint32_t *__restrict__ chunk_off, size_t m,
                                                            size_t mc, size_t n_rows, uint64_t seed, unsigned long long *__restrict__ key) {
  const size_t q = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int lane = lane_id();
  uint32_t j = 0xffffffffu;  // (no item has this index: a lane past the end is a segment of its own kind)
  unsigned long long v = 0;
  bool single = false;
  uint32_t row_len = 0;
  if (q < mc) {
    j = dedup_item_of(chunk_off, m, static_cast<uint32_t>(q));
    const uint32_t row = items[j];
    if (wp_in_bounds(row < n_rows, kSiteDedup)) {
      const uint32_t k = static_cast<uint32_t>(q) - chunk_off[j];
      const size_t r0 = byte_off[row], r1 = byte_off[row + 1];
      const size_t s = r0 + static_cast<size_t>(k) * kDedupChunk;
      const size_t e = min(s + static_cast<size_t>(kDedupChunk), r1);
      if (wp_in_bounds(s < e && e <= n_bytes, kSiteDedup)) {
        single = chunk_off[j + 1] - chunk_off[j] == 1u;
        row_len = static_cast<uint32_t>(r1 - r0);
        uint64_t h = count_mix((count_mix(seed ^ 0x9e3779b97f4a7c15ull) ^ (static_cast<uint64_t>(k) + 1ull)) + 0x632be59bd9b4e019ull);
        const uint32_t words = static_cast<uint32_t>((e - s + 3) >> 2);
        uint32_t i = 0;
        for (; i + 2 <= words; i += 2) {
          const uint64_t x = static_cast<uint64_t>(dedup_word(d32, s, e, i)) | (static_cast<uint64_t>(dedup_word(d32, s, e, i + 1)) << 32);
          h = count_mix(h ^ x) + 0x9e3779b97f4a7c15ull;
        }
        uint64_t x = i < words ? dedup_word(d32, s, e, i) : 0u;
        x |= static_cast<uint64_t>(e - s) << 32;  // (the last word of a chunk has at most 32 bits of data here)
        v = count_mix(h ^ x);
      } else {
        j = 0xffffffffu;
      }
    } else {
      j = 0xffffffffu;
    }
  }
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const unsigned long long t = __shfl_up(v, d, kWave);
    const uint32_t jd = __shfl_up(j, d, kWave);
    if (lane >= d && jd == j) v += t;  // (ascending: equal items d lanes apart are equal in between)
  }
  const uint32_t jn = __shfl_down(j, 1, kWave);
  if (j != 0xffffffffu && (lane == kWave - 1 || jn != j)) {
    if (single) key[j] = dedup_len_mix(seed, row_len) + v;
    else atomicAdd(key + j, v);
  }
}

// key[j] &= mask (a narrowed hash: the sum is masked once it is complete)
__global__ __launch_bounds__(kBlock) void dedup_mask_kernel(uint64_t *__restrict__ key, size_t m, uint64_t mask) {
  const size_t j = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j < m) key[j] &= mask;
}

// Sorted position s: the member's item j = val[s] learns the row of its run's head (head_row[j]), and left[j] = 1 where
// its length differs from the head's — no byte is read for that.  A head is its own head row.
__global__ __launch_bounds__(kBlock) void dedup_match_kernel(const uint32_t *__restrict__ items, const uint32_t *__restrict__ val,
                                                             const uint32_t *__restrict__ head, const uint32_t *__restrict__ run,
                                                             const uint32_t *__restrict__ head_pos, size_t m, size_t n_rows,
                                                             const uint32_t *__restrict__ byte_off, uint32_t *__restrict__ head_row,
                                                             uint32_t *__restrict__ left) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s >= m) return;
  const uint32_t r = run[s] + head[s] - 1u;  // (the exclusive scan counts the heads in front of s)
  const uint32_t j = val[s];
  if (!wp_in_bounds(r < m && j < m, kSiteDedup)) return;
  const uint32_t hs = head_pos[r];
  if (!wp_in_bounds(hs <= s && val[hs] < m, kSiteDedup)) return;
  const uint32_t row = items[j], hrow = items[val[hs]];
  if (!wp_in_bounds(row < n_rows && hrow <= row, kSiteDedup)) return;
  head_row[j] = hrow;
  left[j] = byte_off[row + 1] - byte_off[row] != byte_off[hrow + 1] - byte_off[hrow] ? 1u : 0u;
}

// Chunk q of the round against the same chunk of the head of its item's run: left[item] = 1 where a byte differs.
// Heads (and so single-member runs) and members of another length read nothing.  compared: the bytes of the chunks that
// were compared, summed per wave.
__global__ __launch_bounds__(kBlock) void dedup_compare_kernel(const uint32_t *__restrict__ d32, size_t n_bytes, const uint32_t *__restrict__ byte_off,
                                                               const uint32_t *__restrict__ items, const uint32_t *__restrict__ chunk_off,
                                                               const uint32_t *__restrict__ head_row, size_t m, size_t mc, size_t n_rows,
                                                               uint32_t *__restrict__ left, unsigned long long *__restrict__ compared) {
  const size_t q = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  uint32_t bytes = 0;
  if (q < mc) {
    const uint32_t j = dedup_item_of(chunk_off, m, static_cast<uint32_t>(q));
    const uint32_t row = items[j], hrow = head_row[j];
    if (wp_in_bounds(row < n_rows && hrow <= row, kSiteDedup) && hrow != row) {
      const size_t r0 = byte_off[row], r1 = byte_off[row + 1], h0 = byte_off[hrow], h1 = byte_off[hrow + 1];
      if (r1 - r0 == h1 - h0) {
        const size_t at = static_cast<size_t>(static_cast<uint32_t>(q) - chunk_off[j]) * kDedupChunk;
        const size_t len = min(static_cast<size_t>(kDedupChunk), r1 - r0 - at);
        const size_t s = r0 + at, hs = h0 + at;
        if (wp_in_bounds(at < r1 - r0 && s + len <= n_bytes && hs + len <= n_bytes, kSiteDedup)) {
          const uint32_t words = static_cast<uint32_t>((len + 3) >> 2);
          bool differ = false;
          for (uint32_t i = 0; i < words && !differ; i++) differ = dedup_word(d32, s, s + len, i) != dedup_word(d32, hs, hs + len, i);
          if (differ) left[j] = 1u;
          bytes = static_cast<uint32_t>(len);
        }
      }
    }
  }
  bytes = wave_reduce_sum(bytes);
  if (lane_id() == 0 && bytes != 0) atomicAdd(compared, static_cast<unsigned long long>(bytes));
}

// Sorted position s once the comparison is over: agree[s] = 1 where the member equals the head of its run, and then
// first[row] = the head's row.  agree[m] = 0 closes the array for its scan.
__global__ __launch_bounds__(kBlock) void dedup_settle_kernel(const uint32_t *__restrict__ items, const uint32_t *__restrict__ val,
                                                              const uint32_t *__restrict__ head_row, const uint32_t *__restrict__ left, size_t m,
                                                              size_t n_rows, uint32_t *__restrict__ agree, int32_t *__restrict__ first) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s == 0) agree[m] = 0;
  if (s >= m) return;
  const uint32_t j = val[s];
  uint32_t same = 0;
  if (wp_in_bounds(j < m, kSiteDedup)) {
    const uint32_t row = items[j];
    same = left[j] ? 0u : 1u;
    if (same && wp_in_bounds(row < n_rows, kSiteDedup)) first[row] = static_cast<int32_t>(head_row[j]);
  }
  agree[s] = same;
}

// run r of the round: row_count[its head's row] = the members that agreed (agree_pos: the exclusive scan of agree over
// m + 1 entries).  A row is a head once, in the round that settles it.
__global__ __launch_bounds__(kBlock) void dedup_run_counts_kernel(const uint32_t *__restrict__ items, const uint32_t *__restrict__ val,
                                                                  const uint32_t *__restrict__ head_pos, const uint32_t *__restrict__ agree_pos,
                                                                  const uint32_t *__restrict__ n_runs, size_t m, size_t n_rows,
                                                                  uint32_t *__restrict__ row_count) {
  const size_t r = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (r >= *n_runs || r >= m) return;
  const uint32_t h0 = head_pos[r], h1 = head_pos[r + 1];
  if (!wp_in_bounds(h0 < m && h1 <= m && val[h0] < m, kSiteDedup)) return;
  const uint32_t row = items[val[h0]];
  if (wp_in_bounds(row < n_rows, kSiteDedup)) row_count[row] = agree_pos[h1] - agree_pos[h0];
}

// keep[i] = 1 where row i is the first of its kind; entry n_rows closes the array for its scan
__global__ __launch_bounds__(kBlock) void dedup_keep_kernel(const int32_t *__restrict__ first, size_t n_rows, uint32_t *__restrict__ keep) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i > n_rows) return;
  keep[i] = i < n_rows && first[i] == static_cast<int32_t>(i) ? 1u : 0u;
}

// The table (keep_pos: the exclusive scan of keep): a kept row at its slot with its count and its length in bytes,
// every row with the slot of its first occurrence (inverse, optional).  out_len[n_unique] = 0 closes the lengths.
__global__ __launch_bounds__(kBlock) void dedup_table_kernel(const int32_t *__restrict__ first, const uint32_t *__restrict__ keep_pos,
                                                             const uint32_t *__restrict__ row_count, const uint32_t *__restrict__ byte_off,
                                                             size_t n_rows, size_t n_unique, int32_t *__restrict__ kept,
                                                             long long *__restrict__ counts, int32_t *__restrict__ inverse,
                                                             uint32_t *__restrict__ out_len) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i == 0 && out_len) out_len[n_unique] = 0;
  if (i >= n_rows) return;
  const int32_t f = first[i];
  const bool settled = f >= 0 && static_cast<size_t>(f) <= i;  // (checked in every build: an index follows from it)
  if (!wp_in_bounds(settled, kSiteDedup) || !settled) return;
  const uint32_t k = keep_pos[f];
  if (!wp_in_bounds(k < n_unique, kSiteDedup) || k >= n_unique) return;
  if (inverse) inverse[i] = static_cast<int32_t>(k);
  if (static_cast<size_t>(f) == i) {
    kept[k] = static_cast<int32_t>(i);
    counts[k] = row_count[i];
    if (out_len) out_len[k] = byte_off[i + 1] - byte_off[i];
  }
}

// row_off[k] of the compact form, in elements (out_pos: the exclusive scan of out_len, in bytes); k in [0, n_unique]
__global__ __launch_bounds__(kBlock) void dedup_out_off_kernel(const uint32_t *__restrict__ out_pos, size_t n_unique, uint32_t elem_bytes,
                                                               long long *__restrict__ row_off) {
  const size_t k = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (k > n_unique) return;
  row_off[k] = static_cast<long long>(out_pos[k] / elem_bytes);
}

// The compact data, one lane per 4 output bytes: the kept row of the lane's first byte by bisection in out_pos
// (n_unique + 1 entries, in bytes), the rows of its other bytes by stepping on from there (rows of 1 to 3 bytes share a
// word; at most one kept row is empty), every byte from its place in the input.  The lanes run to the size the host
// knew before the scan (cap, the bytes of the input); *out_bytes ends them.
__global__ __launch_bounds__(kBlock) void dedup_gather_kernel(const uint8_t *__restrict__ data, size_t n_bytes, const uint32_t *__restrict__ byte_off,
                                                              const int32_t *__restrict__ kept, const uint32_t *__restrict__ out_pos,
                                                              size_t n_unique, size_t n_rows, size_t cap, uint32_t *__restrict__ out) {
  const size_t p = (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x) * 4u;
  const size_t total = out_pos[n_unique];
  if (p >= total || p >= cap) return;
  size_t lo = 0, hi = n_unique;  // the last k with out_pos[k] <= p
  while (hi - lo > 1) {
    const size_t mid = (lo + hi) >> 1;
    if (out_pos[mid] <= p) lo = mid; else hi = mid;
  }
  uint32_t w = 0;
  for (uint32_t b = 0; b < 4 && p + b < total; b++) {
    while (lo + 1 < n_unique && out_pos[lo + 1] <= p + b) lo++;
    const int32_t row = kept[lo];
    const bool listed = row >= 0 && static_cast<size_t>(row) < n_rows;
    if (!wp_in_bounds(listed, kSiteDedup) || !listed) continue;
    const size_t at = static_cast<size_t>(byte_off[row]) + (p + b - out_pos[lo]);
    if (wp_in_bounds(at < n_bytes, kSiteDedup) && at < n_bytes) w |= static_cast<uint32_t>(data[at]) << (8u * b);
  }
  out[p >> 2] = w;
}

}  // namespace wp
