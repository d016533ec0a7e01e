// count.h — the kernels of the word counts (include/wordpiece_amd.h, section "word counts"; host path: count_path.h).
// The text is valid UTF-8 (the normalise pre-pass wrote it).  Words are found by class alone: every byte position of a
// tile gets the class byte of the code point that starts there, a word starts at a non-space code point that is a
// spacing character or follows one (or the start of the text), and it ends in front of the next space or word start.
// Starts and ends are compacted by the same tile scan, so the k-th end closes the k-th start and no lane walks a word
// to find its length.  Words are then grouped by a seeded 64-bit hash of their bytes (radix sort, stable, so a run's
// head is its first occurrence), every member is compared with the head of its run byte by byte, and what differs goes
// into the next round with another seed.
#pragma once
#include "common.h"
#include "decode.h"  // class_of_cp
#include "group.h"   // mix64, absorb_bytes, last_le, run_of; the kernels of a grouping round run beside these

namespace wp {

constexpr int kCountItems = 8;                     // byte positions per thread of the word-start pass
constexpr int kCountTile = kBlock * kCountItems;   // T: byte positions per workgroup
constexpr int kCountHalo = 4;                      // bytes in front of a tile that may hold the previous code point
constexpr int kCountMaxWordBytes = 1024;
constexpr uint8_t kCountNoLead = 0xff;             // class slot of a continuation byte or of a position outside the text

// the counters of a call, 64 bits each, in d_scalars from kScalarCount on
enum CountCounter { kCountKeptBytes = 0, kCountCounters = 1 };

// Pass over the byte positions [0, nbytes]: position nbytes stands for the end of the text, where an open word ends.
// WRITE false: per tile the number of word starts and ends.  WRITE true: with the scanned tile counts, the byte position
// of every start and end in text order.
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void count_starts_kernel(const uint8_t *__restrict__ text, size_t nbytes,
                                                              const uint8_t *__restrict__ cls_bmp, uint32_t *__restrict__ tile_starts,
                                                              uint32_t *__restrict__ tile_ends, uint32_t *__restrict__ start,
                                                              uint32_t *__restrict__ end, size_t n_words) {
  __shared__ uint8_t s_b[kCountHalo + kCountTile + 4];  // bytes [base - 4, base + T + 4)
  __shared__ uint8_t s_c[kCountHalo + kCountTile];      // class of the code point that starts at [base - 4, base + T)
  __shared__ uint32_t s_scan[8];
  const size_t base = static_cast<size_t>(blockIdx.x) * kCountTile;
  for (int k = threadIdx.x; k < kCountHalo + kCountTile + 4; k += kBlock) {
    const long long p = static_cast<long long>(base) + k - kCountHalo;
    s_b[k] = (p >= 0 && static_cast<size_t>(p) < nbytes) ? text[p] : 0;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kCountHalo + kCountTile; k += kBlock) {
    const long long p = static_cast<long long>(base) + k - kCountHalo;
    uint8_t f = kCountNoLead;
    const uint32_t b0 = s_b[k];
    if (p >= 0 && static_cast<size_t>(p) < nbytes && (b0 & 0xc0u) != 0x80u) {
      uint32_t cp = b0;
      if (b0 >= 0xf0u) {
        cp = ((b0 & 0x07u) << 18) | ((s_b[k + 1] & 0x3fu) << 12) | ((s_b[k + 2] & 0x3fu) << 6) | (s_b[k + 3] & 0x3fu);
      } else if (b0 >= 0xe0u) {
        cp = ((b0 & 0x0fu) << 12) | ((s_b[k + 1] & 0x3fu) << 6) | (s_b[k + 2] & 0x3fu);
      } else if (b0 >= 0xc0u) {
        cp = ((b0 & 0x1fu) << 6) | (s_b[k + 1] & 0x3fu);
      }
      // (the vocabulary-independent bits alone: the handle's soft list is not consulted)
      f = (cp < 0x110000u ? class_of_cp(cp, cls_bmp, nullptr, 0) : 0) & (kClsSpace | kClsSpacing | kClsPunct);
    }
    s_c[k] = f;
  }
  __syncthreads();
  // the class of the code point in front of this thread's first position: at most 4 bytes back
  const int k0 = kCountHalo + static_cast<int>(threadIdx.x) * kCountItems;
  int prev = -1;  // -1: the start of the text
#pragma unroll
  for (int d = kCountHalo; d >= 1; d--) {
    if (s_c[k0 - d] != kCountNoLead) prev = s_c[k0 - d];
  }
  uint32_t is_start = 0, is_end = 0;  // bit j: position k0 + j
  int pv = prev;
#pragma unroll
  for (int j = 0; j < kCountItems; j++) {
    const size_t p = base + static_cast<size_t>(threadIdx.x) * kCountItems + j;
    const uint8_t f = s_c[k0 + j];
    const bool at_end = p == nbytes;
    if (p > nbytes || (!at_end && f == kCountNoLead)) continue;
    const bool space = at_end || (f & kClsSpace);
    const bool st = !space && (pv < 0 || (f & kClsSpacing) || (pv & kClsSpacing));
    const bool open = pv >= 0 && !(pv & kClsSpace);  // the code point in front belongs to a word
    if (st) is_start |= 1u << j;
    if (open && (space || st)) is_end |= 1u << j;
    pv = at_end ? -1 : f;
  }
  uint32_t tot_s, tot_e;
  const uint32_t ex_s = block_excl_sum(__popc(is_start), s_scan, tot_s);
  const uint32_t ex_e = block_excl_sum(__popc(is_end), s_scan, tot_e);
  if constexpr (!WRITE) {
    if (threadIdx.x == 0) {
      tile_starts[blockIdx.x] = tot_s;
      tile_ends[blockIdx.x] = tot_e;
    }
  } else {
    size_t rs = static_cast<size_t>(tile_starts[blockIdx.x]) + ex_s, re = static_cast<size_t>(tile_ends[blockIdx.x]) + ex_e;
#pragma unroll
    for (int j = 0; j < kCountItems; j++) {
      const uint32_t p = static_cast<uint32_t>(base + static_cast<size_t>(threadIdx.x) * kCountItems + j);
      if (is_start & (1u << j)) {
        if (wp_checked(rs < n_words, kSiteCount)) start[rs] = p;
        rs++;
      }
      if (is_end & (1u << j)) {
        if (wp_checked(re < n_words, kSiteCount)) end[re] = p;
        re++;
      }
    }
  }
}

// flag[w] = 1 where word w is listed (at most max_bytes bytes); word_group[w] = -1 for every word
__global__ __launch_bounds__(kBlock) void count_listed_kernel(const uint32_t *__restrict__ start, const uint32_t *__restrict__ end, size_t n_words,
                                                              uint32_t max_bytes, uint32_t *__restrict__ flag, int32_t *__restrict__ word_group) {
  const size_t w = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (w >= n_words) return;
  flag[w] = end[w] - start[w] <= max_bytes ? 1u : 0u;
  word_group[w] = -1;
}

// key[j] = the seeded hash of the bytes of word items[j], masked; a lane reads at most max_bytes bytes
__global__ __launch_bounds__(kBlock) void count_keys_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ start,
                                                            const uint32_t *__restrict__ end, const uint32_t *__restrict__ items, size_t m,
                                                            uint64_t seed, uint64_t mask, uint32_t max_bytes, uint64_t *__restrict__ key) {
  const size_t j = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j >= m) return;
  const uint32_t w = items[j], b = start[w];
  const uint32_t len = min(end[w] - b, max_bytes);
  key[j] = absorb_bytes(mix64(seed ^ kGolden) ^ len, text + b, len) & mask;
}

// Every member of a run against the run's head, length and bytes (at most max_bytes of them): agree[s] = 1 where they
// are the same word, and the word then belongs to group group_base + run; left[val[s]] = 1 where they differ (by item,
// i.e. in text order).  agree[m] = 0 closes the array for its scan.
__global__ __launch_bounds__(kBlock) void count_verify_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ start,
                                                              const uint32_t *__restrict__ end, const uint32_t *__restrict__ items,
                                                              const uint32_t *__restrict__ val, const uint32_t *__restrict__ head,
                                                              const uint32_t *__restrict__ run, const uint32_t *__restrict__ head_pos, size_t m,
                                                              size_t n_words, uint32_t max_bytes, uint32_t group_base,
                                                              uint32_t *__restrict__ agree, uint32_t *__restrict__ left,
                                                              int32_t *__restrict__ word_group) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s == 0) agree[m] = 0;
  if (s >= m) return;
  const uint32_t r = run_of(head, run, s);
  const uint32_t j = val[s];
  if (!wp_in_bounds(r < m && j < m, kSiteCount)) return;
  const uint32_t hs = head_pos[r];
  if (!wp_in_bounds(hs <= s && val[hs] < m, kSiteCount)) return;
  const uint32_t w = items[j], hw = items[val[hs]];
  if (!wp_in_bounds(w < n_words && hw < n_words, kSiteCount)) return;
  bool same = true;
  if (hs != s) {
    const uint32_t a = start[w], b = start[hw], len = end[w] - a;
    same = len == end[hw] - b;
    if (same) {
      const uint32_t lim = min(len, max_bytes);
      for (uint32_t i = 0; i < lim; i++) {
        if (text[a + i] != text[b + i]) {
          same = false;
          break;
        }
      }
    }
  }
  agree[s] = same ? 1u : 0u;
  left[j] = same ? 0u : 1u;
  if (same) word_group[w] = static_cast<int32_t>(group_base + r);
}

// group r of the round: its first word (the head of the run: the sort is stable and the items ascend) and its count, the
// number of members that agreed (agree_pos: the exclusive scan of agree over m + 1 entries)
__global__ __launch_bounds__(kBlock) void count_groups_kernel(const uint32_t *__restrict__ items, const uint32_t *__restrict__ val,
                                                              const uint32_t *__restrict__ head_pos, const uint32_t *__restrict__ agree_pos,
                                                              const uint32_t *__restrict__ n_runs, size_t m, uint32_t *__restrict__ group_first,
                                                              uint32_t *__restrict__ group_count) {
  const size_t r = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (r >= *n_runs || r >= m) return;
  const uint32_t h0 = head_pos[r], h1 = head_pos[r + 1];
  if (!wp_in_bounds(h0 < m && h1 <= m && val[h0] < m, kSiteCount)) return;
  group_first[r] = items[val[h0]];
  group_count[r] = agree_pos[h1] - agree_pos[h0];
}

// keep[g] = 1 where the group's count reaches min_count; the bytes of the kept words summed into *kept_bytes
__global__ __launch_bounds__(kBlock) void count_filter_kernel(const uint32_t *__restrict__ group_first, const uint32_t *__restrict__ group_count,
                                                              size_t n_groups, unsigned long long min_count, const uint32_t *__restrict__ start,
                                                              const uint32_t *__restrict__ end, uint32_t *__restrict__ keep,
                                                              unsigned long long *__restrict__ kept_bytes) {
  const size_t g = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  unsigned long long bytes = 0;
  if (g < n_groups) {
    const bool k = group_count[g] >= min_count;
    keep[g] = k ? 1u : 0u;
    if (k) bytes = end[group_first[g]] - start[group_first[g]];
  }
  bytes = wave_reduce_sum64(bytes);
  if (lane_id() == 0 && bytes != 0) atomicAdd(kept_bytes, bytes);
}

// the sort key of every kept group at its compacted slot, and the group it stands for: the first word (order 0), or
// the count descending in the high half with the first word below it (order 1)
__global__ __launch_bounds__(kBlock) void count_order_keys_kernel(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ keep_pos,
                                                                  const uint32_t *__restrict__ group_first, const uint32_t *__restrict__ group_count,
                                                                  size_t n_groups, size_t n_kept, int by_count, uint64_t *__restrict__ key,
                                                                  uint32_t *__restrict__ kept_group) {
  const size_t g = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (g >= n_groups || !keep[g]) return;
  const uint32_t c = keep_pos[g];
  if (!wp_in_bounds(c < n_kept, kSiteCount)) return;
  kept_group[c] = static_cast<uint32_t>(g);
  key[c] = by_count ? (static_cast<uint64_t>(0xffffffffu - group_count[g]) << 32) | group_first[g] : static_cast<uint64_t>(group_first[g]);
}

// table entry t (the sorted order): count, length and source of its word; the group learns its final index.
// len[n_kept] = 0 closes the lengths for their scan.
__global__ __launch_bounds__(kBlock) void count_emit_kernel(const uint32_t *__restrict__ val, const uint32_t *__restrict__ kept_group,
                                                            const uint32_t *__restrict__ group_first, const uint32_t *__restrict__ group_count,
                                                            const uint32_t *__restrict__ start, const uint32_t *__restrict__ end, size_t n_kept,
                                                            size_t n_groups, long long *__restrict__ counts, uint32_t *__restrict__ len,
                                                            uint32_t *__restrict__ src, int32_t *__restrict__ group_final) {
  const size_t t = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (t == 0) len[n_kept] = 0;
  if (t >= n_kept) return;
  const uint32_t c = val[t];
  if (!wp_in_bounds(c < n_kept, kSiteCount)) return;
  const uint32_t g = kept_group[c];
  if (!wp_in_bounds(g < n_groups, kSiteCount)) return;
  const uint32_t w = group_first[g];
  counts[t] = group_count[g];
  len[t] = end[w] - start[w];
  src[t] = start[w];
  group_final[g] = static_cast<int32_t>(t);
}

// The pool, one byte per lane and consecutive lanes on consecutive bytes: the word of byte p is found by bisection in
// word_off (group_offsets_kernel wrote it), its byte comes from the text, and the last byte of a word's slot is the terminator.
__global__ __launch_bounds__(kBlock) void count_gather_kernel(const uint8_t *__restrict__ text, size_t text_bytes, const long long *__restrict__ word_off,
                                                              const uint32_t *__restrict__ src, size_t n_kept, int terminator, size_t pool_bytes,
                                                              uint8_t *__restrict__ pool) {
  const size_t p = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (p >= pool_bytes) return;
  const size_t lo = last_le(word_off, size_t(0), n_kept, p);
  const size_t k = p - static_cast<size_t>(word_off[lo]);
  uint8_t b;
  if (terminator >= 0 && p + 1 == static_cast<size_t>(word_off[lo + 1])) {
    b = static_cast<uint8_t>(terminator);
  } else {
    const size_t at = static_cast<size_t>(src[lo]) + k;
    b = wp_in_bounds(at < text_bytes, kSiteCount) ? text[at] : 0;
  }
  pool[p] = b;
}

// word_index[w] = the table entry of word w's group, -1 where the word is long or its group was dropped
__global__ __launch_bounds__(kBlock) void count_index_kernel(const int32_t *__restrict__ word_group, const int32_t *__restrict__ group_final,
                                                             size_t n_words, size_t n_groups, int32_t *__restrict__ word_index) {
  const size_t w = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (w >= n_words) return;
  const int32_t g = word_group[w];
  int32_t t = -1;
  if (g >= 0 && wp_in_bounds(static_cast<size_t>(g) < n_groups, kSiteCount)) t = group_final[g];
  word_index[w] = t;
}

}  // namespace wp
