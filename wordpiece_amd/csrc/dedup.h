// dedup.h — the kernels of the duplicate-row removal (include/wordpiece_amd.h, section "duplicate rows"; host path:
// dedup_path.h).  The input is a ragged batch: a flat element stream (1 or 4 bytes per element) and row_off.  Every row
// is cut into chunks of kDedupChunk bytes, and all work on bytes is flat over the chunk list: a chunk finds its row by
// bisection in the chunk offsets, so one row of 10^8 bytes costs what 10^6 rows of 100 do, and no lane, wave or
// workgroup walks a row.  The key of a row is the sum mod 2^64 of the seeded hashes of its chunks (each mixed with its
// index in the row) plus a mix of the length: an integer sum, whatever order the chunks arrive in.  Rows are then grouped
// as count.h groups words (stable radix sort of the keys, run heads, head positions: the kernels of group.h), every
// member is compared with the head of its run chunk by chunk, and what differs goes into the next round under another
// seed.  The sort is stable and the item list ascends, so the head of a run is its smallest row: the first occurrence.
#pragma once
#include "common.h"
#include "group.h"  // mix64, word_at, same_words, last_le, run_of, ragged_row; its kernels run beside these

namespace wp {

constexpr int kDedupChunk = 256;                    // C: bytes of a chunk (a multiple of 8)
constexpr int kDedupTile = kBlock * kDedupChunk;    // bytes a workgroup of the key and compare kernels covers

// the counters of a call, 64 bits each, in d_scalars from kScalarDedup on
enum DedupCounter { kDedupEmpty = 0, kDedupCompared = 1, kDedupCounters = 4 };

// the mix of a row's length in bytes under the round's seed: what the chunk values are added to
__device__ __forceinline__ uint64_t dedup_len_mix(uint64_t seed, uint32_t len) {
  return mix64(mix64(seed ^ kGolden) ^ (static_cast<uint64_t>(len) | (1ull << 40)));
}

// Row i through ragged_row (offsets checked, byte_off, *n_elems), then its chunks and the row as item i of round 0.
// Entry n_rows closes n_chunks (0) for its scan.  Counted: the empty rows.
__global__ __launch_bounds__(kBlock) void dedup_rows_kernel(const long long *__restrict__ row_off, size_t n_rows, uint32_t elem_bytes,
                                                            uint32_t *__restrict__ byte_off, uint32_t *__restrict__ n_chunks,
                                                            uint32_t *__restrict__ items, int32_t *__restrict__ first,
                                                            uint32_t *__restrict__ bad, unsigned long long *__restrict__ n_elems,
                                                            unsigned long long *__restrict__ counters) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  bool empty = false;
  if (i <= n_rows) {
    const RaggedRow r = ragged_row(row_off, n_rows, elem_bytes, i, byte_off, bad, n_elems);
    if (!r.row) {
      n_chunks[i] = 0;
    } else {
      const unsigned long long ch = r.len > 0xffffffffull ? 0xffffffffull : (r.len * elem_bytes + kDedupChunk - 1) / kDedupChunk;
      n_chunks[i] = static_cast<uint32_t>(ch > 0xffffffffull ? 0xffffffffull : ch);
      items[i] = static_cast<uint32_t>(i);
      first[i] = -1;
      empty = r.len == 0;  // (a row whose offsets descend is a bad row: the call fails before this count is read)
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

// Chunk q of the round (mc of them, laid out item by item; its item: the last j with chunk_off[j] <= q, chunk_off
// has m + 1 entries and chunk_off[m] > q): the seeded hash of its at most C bytes, its index in the row mixed in.  The
// values of one item are summed inside the wave by a segmented scan (the lanes of a wave ascend in q, so in item) and
// leave it as one 64-bit atomic per wave and item segment; an item of one chunk stores its key without an atomic.  The
// number of chunks stays below 2^32: n_bytes <= UINT32_MAX and n_rows < 2^31 bound it by 2^24 + 2^31.
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
    j = static_cast<uint32_t>(last_le(chunk_off, size_t(0), m, q));
    const uint32_t row = items[j];
    if (wp_in_bounds(row < n_rows, kSiteDedup)) {
      const uint32_t k = static_cast<uint32_t>(q) - chunk_off[j];
      const size_t r0 = byte_off[row], r1 = byte_off[row + 1];
      const size_t s = r0 + static_cast<size_t>(k) * kDedupChunk;
      const size_t e = min(s + static_cast<size_t>(kDedupChunk), r1);
      if (wp_in_bounds(s < e && e <= n_bytes, kSiteDedup)) {
        single = chunk_off[j + 1] - chunk_off[j] == 1u;
        row_len = static_cast<uint32_t>(r1 - r0);
        uint64_t h = mix64((mix64(seed ^ kGolden) ^ (static_cast<uint64_t>(k) + 1ull)) + 0x632be59bd9b4e019ull);
        const uint32_t words = static_cast<uint32_t>((e - s + 3) >> 2);
        uint32_t i = 0;
        for (; i + 2 <= words; i += 2) {
          const uint64_t x = static_cast<uint64_t>(word_at(d32, s, e, i)) | (static_cast<uint64_t>(word_at(d32, s, e, i + 1)) << 32);
          h = mix64(h ^ x) + kGolden;
        }
        uint64_t x = i < words ? word_at(d32, s, e, i) : 0u;
        x |= static_cast<uint64_t>(e - s) << 32;  // (the last word of a chunk has at most 32 bits of data here)
        v = mix64(h ^ x);
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
  const uint32_t r = run_of(head, run, s);
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
    const uint32_t j = static_cast<uint32_t>(last_le(chunk_off, size_t(0), m, q));
    const uint32_t row = items[j], hrow = head_row[j];
    if (wp_in_bounds(row < n_rows && hrow <= row, kSiteDedup) && hrow != row) {
      const size_t r0 = byte_off[row], r1 = byte_off[row + 1], h0 = byte_off[hrow], h1 = byte_off[hrow + 1];
      if (r1 - r0 == h1 - h0) {
        const size_t at = static_cast<size_t>(static_cast<uint32_t>(q) - chunk_off[j]) * kDedupChunk;
        const size_t len = min(static_cast<size_t>(kDedupChunk), r1 - r0 - at);
        const size_t s = r0 + at, hs = h0 + at;
        if (wp_in_bounds(at < r1 - r0 && s + len <= n_bytes && hs + len <= n_bytes, kSiteDedup)) {
          if (!same_words(d32, s, d32, hs, static_cast<uint32_t>(len))) left[j] = 1u;
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

}  // namespace wp
