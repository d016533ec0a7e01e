// learn.h — the kernels of the vocabulary learner (include/wordpiece_amd.h, section "vocabulary learner"; host path:
// learn_path.h).  The input is a word table: a byte pool, word_off, counts.  A word that passes the filters has L <= 64
// code points and L + 1 cells (the byte position of every code point and of its end), and stands for L (L + 1) / 2
// items: its substrings [s, e) in the order (s, e).  An item is an occurrence of the token (s > 0, bytes).  Items are
// grouped into tokens as count.h groups words: a seeded 64-bit hash of flag and bytes, a stable radix sort, every member
// against the head of its run, what differs into the next round.  Item i - 1 is item i's prefix one code point shorter
// whenever e - 1 > s, so a group's parent group (its token without the last code point) is the group of the item in
// front of its first item.  One threshold of the search is then: the sum of the word counts of the items whose start is
// active, per group, over the items sorted by group; and one launch per token length, longest first, that keeps the
// groups that reach the threshold and takes their count from every group up the parent chain.
#pragma once
#include "common.h"
#include "group.h"  // mix64, absorb_bytes, last_le, run_of; the kernels of a grouping round run beside these

namespace wp {

constexpr int kLearnMaxChars = 64;
constexpr uint32_t kLearnCps = 0x110000u;  // slots of the per-code-point tables

// what the table check found in word w: kLearnBad key = w << 3 | kind, the smallest wins (~0: nothing)
enum LearnBad { kLearnBadOffsets = 1, kLearnBadCount = 2, kLearnBadUtf8 = 3 };
// the counters of a call, 64 bits each, in d_scalars from kScalarLearn on
enum LearnCounter { kLearnReserved = 0, kLearnLong = 1, kLearnCharDropped = 2, kLearnCounters = 4 };

// entries of the list: where the text of an entry comes from
constexpr uint32_t kLearnFromReserved = 0, kLearnFromCp = 1, kLearnFromPool = 2;

__device__ __forceinline__ void learn_count(unsigned long long *counters, int which, bool hit) {
  const uint32_t n = wave_reduce_sum(hit ? 1u : 0u);
  if (lane_id() == 0 && n != 0) atomicAdd(counters + which, static_cast<unsigned long long>(n));
}

// Word w of the table: its offsets, its count and its bytes checked, and wlen[w] = its code points where it passes the
// filters that need no other word (not empty, no reserved token, no "##" in front, at most max_chars), else 0.
__global__ __launch_bounds__(kBlock) void learn_words_kernel(const uint8_t *__restrict__ pool, size_t pool_bytes, const long long *__restrict__ word_off,
                                                             const long long *__restrict__ counts, size_t n_words, int term,
                                                             const uint8_t *__restrict__ res, const uint32_t *__restrict__ res_off, int n_res,
                                                             uint32_t max_chars, uint32_t *__restrict__ wlen,
                                                             unsigned long long *__restrict__ bad, unsigned long long *__restrict__ counters) {
  const size_t w = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  bool reserved = false, too_long = false;
  if (w < n_words) {
    const long long a = word_off[w], b = word_off[w + 1];
    int kind = 0;
    uint32_t len = 0;
    if (a < 0 || b < a + term || static_cast<unsigned long long>(b) > pool_bytes) {
      kind = kLearnBadOffsets;
    } else {
      if (counts[w] < 0) kind = kLearnBadCount;
      const uint8_t *p = pool + a;
      const long long nb = b - a - term;
      long long i = 0;
      while (i < nb) {
        const uint32_t cp = decode_one(p + i, nb - i);
        if (cp == kInvalidUnicode) {
          if (kind == 0) kind = kLearnBadUtf8;
          break;
        }
        i += cp < 0x80u ? 1 : cp < 0x800u ? 2 : cp < 0x10000u ? 3 : 4;
        if (len <= max_chars) len++;
      }
      if (kind == 0 && nb != 0) {
        reserved = nb >= 2 && p[0] == '#' && p[1] == '#';
        for (int r = 0; r < n_res && !reserved; r++) {
          const uint32_t ra = res_off[r], rn = res_off[r + 1] - ra;
          if (rn != static_cast<unsigned long long>(nb)) continue;
          bool same = true;
          for (uint32_t k = 0; k < rn && same; k++) same = res[ra + k] == p[k];
          reserved = same;
        }
        too_long = !reserved && len > max_chars;
      }
    }
    if (kind != 0) atomicMin(bad, (static_cast<unsigned long long>(w) << 3) | static_cast<unsigned long long>(kind));
    wlen[w] = (kind == 0 && !reserved && !too_long) ? len : 0u;
  }
  learn_count(counters, kLearnReserved, reserved);
  learn_count(counters, kLearnLong, too_long);
}

// the code points of the remaining words: present[cp] = 1, and occ[cp] (optional) += the word's count
__global__ __launch_bounds__(kBlock) void learn_chars_kernel(const uint8_t *__restrict__ pool, const long long *__restrict__ word_off,
                                                             const long long *__restrict__ counts, const uint32_t *__restrict__ wlen, size_t n_words,
                                                             uint32_t *__restrict__ present, unsigned long long *__restrict__ occ) {
  const size_t w = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (w >= n_words) return;
  const uint32_t n = wlen[w];
  const uint8_t *p = pool + word_off[w];
  const unsigned long long c = static_cast<unsigned long long>(counts[w]);
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t cp = decode_one(p, 4);  // (checked: valid, and the word ends no earlier)
    p += cp < 0x80u ? 1 : cp < 0x800u ? 2 : cp < 0x10000u ? 3 : 4;
    if (!wp_in_bounds(cp < kLearnCps, kSiteLearn)) continue;
    present[cp] = 1u;
    if (occ && c != 0) atomicAdd(occ + cp, c);
  }
}

// the present code points in ascending order with their occurrences (pos: the exclusive scan of present)
__global__ __launch_bounds__(kBlock) void learn_char_list_kernel(const uint32_t *__restrict__ present, const uint32_t *__restrict__ pos,
                                                                 const unsigned long long *__restrict__ occ, size_t cap, uint32_t *__restrict__ char_cp,
                                                                 uint64_t *__restrict__ rank_key) {
  const uint32_t cp = blockIdx.x * kBlock + threadIdx.x;
  if (cp >= kLearnCps || !present[cp]) return;
  const uint32_t k = pos[cp];
  if (!wp_in_bounds(k < cap, kSiteLearn)) return;
  char_cp[k] = cp;
  if (rank_key) rank_key[k] = ~static_cast<uint64_t>(occ[cp]);  // (ascending: the most frequent first; stable: ties by code point)
}

// allowed[cp] = 1 for the first `allow` characters of the ranking (val: the list slots in rank order)
__global__ __launch_bounds__(kBlock) void learn_allow_kernel(const uint32_t *__restrict__ val, const uint32_t *__restrict__ char_cp, size_t n_chars,
                                                             size_t allow, uint32_t *__restrict__ allowed) {
  const size_t r = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (r >= allow || r >= n_chars) return;
  const uint32_t k = val[r];
  if (!wp_in_bounds(k < n_chars, kSiteLearn)) return;
  allowed[char_cp[k]] = 1u;
}

// a remaining word that holds a character outside the allowed ones is dropped
__global__ __launch_bounds__(kBlock) void learn_char_filter_kernel(const uint8_t *__restrict__ pool, const long long *__restrict__ word_off,
                                                                   size_t n_words, const uint32_t *__restrict__ allowed, uint32_t *__restrict__ wlen,
                                                                   unsigned long long *__restrict__ counters) {
  const size_t w = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  bool drop = false;
  if (w < n_words) {
    const uint32_t n = wlen[w];
    const uint8_t *p = pool + word_off[w];
    for (uint32_t k = 0; k < n && !drop; k++) {
      const uint32_t cp = decode_one(p, 4);
      p += cp < 0x80u ? 1 : cp < 0x800u ? 2 : cp < 0x10000u ? 3 : 4;
      drop = cp >= kLearnCps || !allowed[cp];
    }
    if (drop) wlen[w] = 0u;
  }
  learn_count(counters, kLearnCharDropped, drop);
}

// items[w] = L (L + 1) / 2 and cells[w] = L + 1 of a remaining word, 0 of any other; entry n_words closes both for their scans
__global__ __launch_bounds__(kBlock) void learn_sizes_kernel(const uint32_t *__restrict__ wlen, size_t n_words, uint32_t *__restrict__ items,
                                                             uint32_t *__restrict__ cells) {
  const size_t w = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (w > n_words) return;
  const uint32_t n = w < n_words ? wlen[w] : 0u;
  items[w] = n * (n + 1u) / 2u;
  cells[w] = n ? n + 1u : 0u;
}

// cell[cell_off[w] + k] = the byte position in the pool of code point k of word w, k = L: of its end
__global__ __launch_bounds__(kBlock) void learn_cells_kernel(const uint8_t *__restrict__ pool, const long long *__restrict__ word_off,
                                                             const uint32_t *__restrict__ wlen, const uint32_t *__restrict__ cell_off, size_t n_words,
                                                             size_t n_cells, uint32_t *__restrict__ cell) {
  const size_t w = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (w >= n_words) return;
  const uint32_t n = wlen[w];
  if (n == 0) return;
  const size_t co = cell_off[w];
  if (!wp_in_bounds(co + n < n_cells, kSiteLearn)) return;
  uint32_t at = static_cast<uint32_t>(word_off[w]);
  for (uint32_t k = 0; k < n; k++) {
    cell[co + k] = at;
    const uint32_t b0 = pool[at];
    at += b0 < 0x80u ? 1 : b0 < 0xe0u ? 2 : b0 < 0xf0u ? 3 : 4;
  }
  cell[co + n] = at;
}

// item i: its word by bisection in item_off (n_words + 1 entries), then s and e from its place among the word's items
__global__ __launch_bounds__(kBlock) void learn_items_kernel(const uint32_t *__restrict__ item_off, const uint32_t *__restrict__ wlen, size_t n_words,
                                                             size_t n_items, uint32_t *__restrict__ item_word, uint16_t *__restrict__ item_se,
                                                             uint32_t *__restrict__ list) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n_items) return;
  const size_t lo = last_le(item_off, size_t(0), n_words, i);
  const uint32_t n = wlen[lo];
  uint32_t r = static_cast<uint32_t>(i - item_off[lo]), s = 0;
  while (s < n && r >= n - s) {
    r -= n - s;
    s++;
  }
  if (!wp_in_bounds(s < n && s + 1 + r <= n, kSiteLearn)) {
    s = 0;
    r = 0;
  }
  item_word[i] = static_cast<uint32_t>(lo);
  item_se[i] = static_cast<uint16_t>(s | ((s + 1 + r) << 8));
  list[i] = static_cast<uint32_t>(i);
}

// the byte range and the flag of item i
struct LearnSpan {
  uint32_t a, b, joined;
};
__device__ __forceinline__ LearnSpan learn_span(uint32_t i, const uint32_t *__restrict__ item_word, const uint16_t *__restrict__ item_se,
                                                const uint32_t *__restrict__ cell_off, const uint32_t *__restrict__ cell) {
  const uint32_t se = item_se[i], s = se & 0xffu, e = se >> 8;
  const uint32_t co = cell_off[item_word[i]];
  return LearnSpan{cell[co + s], cell[co + e], s != 0 ? 1u : 0u};
}

// key[j] = the seeded hash of flag and bytes of item list[j], masked
__global__ __launch_bounds__(kBlock) void learn_keys_kernel(const uint8_t *__restrict__ pool, const uint32_t *__restrict__ item_word,
                                                            const uint16_t *__restrict__ item_se, const uint32_t *__restrict__ cell_off,
                                                            const uint32_t *__restrict__ cell, const uint32_t *__restrict__ list, size_t m,
                                                            size_t n_items, uint64_t seed, uint64_t mask, uint64_t *__restrict__ key) {
  const size_t j = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j >= m) return;
  const uint32_t it = list[j];
  if (!wp_in_bounds(it < n_items, kSiteLearn)) {
    key[j] = 0;
    return;
  }
  const LearnSpan sp = learn_span(it, item_word, item_se, cell_off, cell);
  const uint32_t len = sp.b - sp.a;
  // (length and flag are mixed before the first bytes come in: xored into the same word, the flag would cancel against
  // a bit of the text, and "##abcdb" would collide with "abcdc")
  const uint64_t h = mix64(mix64(seed ^ kGolden) ^ (static_cast<uint64_t>(len) | (static_cast<uint64_t>(sp.joined) << 32)));
  key[j] = absorb_bytes(h, pool + sp.a, len) & mask;
}

// Every member of a run against the run's head: flag, length, then bytes.  Where they agree the item belongs to group
// group_base + run; left[val[s]] = 1 where they differ (by list slot, i.e. in item order).
__global__ __launch_bounds__(kBlock) void learn_verify_kernel(const uint8_t *__restrict__ pool, const uint32_t *__restrict__ item_word,
                                                              const uint16_t *__restrict__ item_se, const uint32_t *__restrict__ cell_off,
                                                              const uint32_t *__restrict__ cell, const uint32_t *__restrict__ list,
                                                              const uint32_t *__restrict__ val, const uint32_t *__restrict__ head,
                                                              const uint32_t *__restrict__ run, const uint32_t *__restrict__ head_pos, size_t m,
                                                              size_t n_items, uint32_t group_base, uint32_t *__restrict__ left,
                                                              int32_t *__restrict__ item_group) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s >= m) return;
  const uint32_t r = run_of(head, run, s);
  const uint32_t j = val[s];
  if (!wp_in_bounds(r < m && j < m, kSiteLearn)) return;
  const uint32_t hs = head_pos[r];
  if (!wp_in_bounds(hs <= s && val[hs] < m, kSiteLearn)) return;
  const uint32_t it = list[j], hit = list[val[hs]];
  if (!wp_in_bounds(it < n_items && hit < n_items, kSiteLearn)) return;
  bool same = true;
  if (hs != s) {
    const LearnSpan x = learn_span(it, item_word, item_se, cell_off, cell), y = learn_span(hit, item_word, item_se, cell_off, cell);
    const uint32_t len = x.b - x.a;
    same = x.joined == y.joined && len == y.b - y.a;
    for (uint32_t i = 0; same && i < len; i++) same = pool[x.a + i] == pool[y.a + i];
  }
  left[j] = same ? 0u : 1u;
  if (same) item_group[it] = static_cast<int32_t>(group_base + r);
}

// group r of the round: its first item (the head of the run: the sort is stable and the list ascends)
__global__ __launch_bounds__(kBlock) void learn_group_first_kernel(const uint32_t *__restrict__ list, const uint32_t *__restrict__ val,
                                                                   const uint32_t *__restrict__ head_pos, const uint32_t *__restrict__ n_runs, size_t m,
                                                                   uint32_t *__restrict__ group_first) {
  const size_t r = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (r >= *n_runs || r >= m) return;
  const uint32_t h0 = head_pos[r];
  if (!wp_in_bounds(h0 < m && val[h0] < m, kSiteLearn)) return;
  group_first[r] = list[val[h0]];
}

// group g: its length in code points as the key of the level sort, and its parent group (-1: a single character)
__global__ __launch_bounds__(kBlock) void learn_group_info_kernel(const uint32_t *__restrict__ group_first, const uint16_t *__restrict__ item_se,
                                                                  const int32_t *__restrict__ item_group, size_t n_groups, size_t n_items,
                                                                  uint64_t *__restrict__ len_key, int32_t *__restrict__ parent) {
  const size_t g = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (g >= n_groups) return;
  const uint32_t i = group_first[g];
  uint32_t len = 1;
  int32_t par = -1;
  if (wp_in_bounds(i < n_items, kSiteLearn)) {
    const uint32_t se = item_se[i];
    len = (se >> 8) - (se & 0xffu);
    if (len > 1) par = item_group[i - 1];  // (item i - 1: the same word and start, one code point shorter)
    if (!wp_in_bounds(par < static_cast<int32_t>(n_groups), kSiteLearn)) par = -1;
  }
  len_key[g] = len;
  parent[g] = par;
}

// bounds[L] / bounds[65 + L]: where the groups of length L begin and end in the order of the level sort (cleared before)
__global__ __launch_bounds__(kBlock) void learn_level_bounds_kernel(const uint64_t *__restrict__ len_key, size_t n_groups, uint32_t *__restrict__ bounds) {
  const size_t p = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (p >= n_groups) return;
  const uint64_t len = len_key[p];
  if (!wp_in_bounds(len >= 1 && len <= kLearnMaxChars, kSiteLearn)) return;
  if (p == 0 || len_key[p - 1] != len) bounds[len] = static_cast<uint32_t>(p);
  if (p + 1 == n_groups || len_key[p + 1] != len) bounds[kLearnMaxChars + 1 + len] = static_cast<uint32_t>(p + 1);
}

// key[i] = the group of item i (the sort behind it lays the items out group by group)
__global__ __launch_bounds__(kBlock) void learn_group_keys_kernel(const int32_t *__restrict__ item_group, size_t n_items, uint64_t *__restrict__ key) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n_items) return;
  key[i] = static_cast<uint64_t>(static_cast<uint32_t>(item_group[i]));
}

// char_group[2 k + joined] = the group of the single character char_cp[k], bare or joined (cleared to -1 before)
__global__ __launch_bounds__(kBlock) void learn_char_groups_kernel(const uint8_t *__restrict__ pool, const uint32_t *__restrict__ level_groups, size_t n,
                                                                   const uint32_t *__restrict__ group_first, const uint32_t *__restrict__ item_word,
                                                                   const uint16_t *__restrict__ item_se, const uint32_t *__restrict__ cell_off,
                                                                   const uint32_t *__restrict__ cell, const uint32_t *__restrict__ char_cp, size_t n_chars,
                                                                   size_t n_groups, size_t n_items, int32_t *__restrict__ char_group) {
  const size_t p = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (p >= n) return;
  const uint32_t g = level_groups[p];
  if (!wp_in_bounds(g < n_groups && group_first[g] < n_items, kSiteLearn)) return;
  const LearnSpan sp = learn_span(group_first[g], item_word, item_se, cell_off, cell);
  const uint32_t cp = decode_one(pool + sp.a, 4);
  const size_t lo = last_le(char_cp, size_t(0), n_chars, cp);  // (char_cp ascends: the slot of cp, if it is listed)
  if (!wp_in_bounds(n_chars != 0 && char_cp[lo] == cp, kSiteLearn)) return;
  char_group[2 * lo + sp.joined] = static_cast<int32_t>(g);
}

// The greedy longest-match split of every remaining word over the kept tokens of the iteration before: active[cell] = 1
// at the start of every piece.  The item of (w, s, e) is item_off[w] + s L - s (s - 1) / 2 + e - s - 1; a single
// character always matches.
__global__ __launch_bounds__(kBlock) void learn_split_kernel(const uint32_t *__restrict__ wlen, const uint32_t *__restrict__ item_off,
                                                             const uint32_t *__restrict__ cell_off, const int32_t *__restrict__ item_group,
                                                             const uint32_t *__restrict__ kept, size_t n_words, size_t n_items, size_t n_groups,
                                                             size_t n_cells, uint8_t *__restrict__ active) {
  const size_t w = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (w >= n_words) return;
  const uint32_t n = wlen[w];
  if (n == 0) return;
  const size_t co = cell_off[w], io = item_off[w];
  if (!wp_in_bounds(co + n < n_cells, kSiteLearn)) return;
  for (uint32_t k = 0; k <= n; k++) active[co + k] = 0;
  uint32_t p = 0;
  while (p < n) {
    active[co + p] = 1;
    const size_t row = io + static_cast<size_t>(p) * n - (p ? static_cast<size_t>(p) * (p - 1u) / 2u : 0u);
    uint32_t e = n;
    for (; e > p + 1; e--) {
      const size_t i = row + (e - p - 1);
      if (!wp_in_bounds(i < n_items, kSiteLearn)) continue;
      const int32_t g = item_group[i];
      if (wp_in_bounds(g >= 0 && static_cast<size_t>(g) < n_groups, kSiteLearn) && kept[g]) break;
    }
    p = e;
  }
}

// The sum of the word counts of the active items per group, over the items sorted by group (perm: the item at a sorted
// position; gkey: its group): a segmented scan inside the wave, then one 64-bit atomic per wave and run segment.
// active == nullptr: every start is active (iteration 0).
__global__ __launch_bounds__(kBlock) void learn_sum_kernel(const uint32_t *__restrict__ perm, const uint64_t *__restrict__ gkey,
                                                           const uint32_t *__restrict__ item_word, const uint16_t *__restrict__ item_se,
                                                           const uint32_t *__restrict__ cell_off, const long long *__restrict__ counts,
                                                           const uint8_t *__restrict__ active, size_t n_items, size_t n_groups,
                                                           unsigned long long *__restrict__ sum) {
  const size_t p = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int lane = lane_id();
  unsigned long long v = 0;
  uint32_t g = 0xffffffffu;  // (no lane of the text has this group: a lane past the end is a segment of its own kind)
  if (p < n_items) {
    const uint32_t i = perm[p];
    g = static_cast<uint32_t>(gkey[p]);
    if (wp_in_bounds(i < n_items && g < n_groups, kSiteLearn)) {
      const uint32_t w = item_word[i];
      if (!active || active[cell_off[w] + (item_se[i] & 0xffu)]) v = static_cast<unsigned long long>(counts[w]);
    } else {
      g = 0xffffffffu;
    }
  }
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const unsigned long long t = __shfl_up(v, d, kWave);
    const uint32_t gd = __shfl_up(g, d, kWave);
    if (lane >= d && gd == g) v += t;  // (sorted: equal groups d lanes apart are equal in between)
  }
  const uint32_t gn = __shfl_down(g, 1, kWave);
  if (g != 0xffffffffu && (lane == kWave - 1 || gn != g) && v != 0) atomicAdd(sum + g, v);
}

// The groups of one length (level: their slice of the level order): a group whose count reaches the threshold is kept,
// and its count leaves every group up its parent chain.  n_kept (optional): the kept groups, counted per wave.
__global__ __launch_bounds__(kBlock) void learn_level_kernel(const uint32_t *__restrict__ level, size_t n, long long thresh, size_t n_groups,
                                                             const int32_t *__restrict__ parent, unsigned long long *__restrict__ sum,
                                                             uint32_t *__restrict__ kept, uint32_t *__restrict__ n_kept) {
  const size_t p = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  bool keep = false;
  if (p < n) {
    const uint32_t g = level[p];
    if (wp_in_bounds(g < n_groups, kSiteLearn)) {
      const long long c = static_cast<long long>(sum[g]);
      keep = c >= thresh;
      kept[g] = keep ? 1u : 0u;
      if (keep) {
        int32_t q = parent[g];
        for (int hop = 0; q >= 0 && hop < kLearnMaxChars; hop++) {
          atomicAdd(sum + q, 0ull - static_cast<unsigned long long>(c));  // (two's complement: counts may go negative)
          q = parent[q];
        }
      }
    }
  }
  if (n_kept) {
    const uint32_t k = wave_reduce_sum(keep ? 1u : 0u);
    if (lane_id() == 0 && k != 0) atomicAdd(n_kept, k);
  }
}

// flag[g] = 1 where group g goes into the list behind the characters: kept, and longer than one character
__global__ __launch_bounds__(kBlock) void learn_listed_kernel(const uint32_t *__restrict__ kept, const int32_t *__restrict__ parent, size_t n_groups,
                                                              uint32_t *__restrict__ flag) {
  const size_t g = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (g >= n_groups) return;
  flag[g] = (kept[g] && parent[g] >= 0) ? 1u : 0u;
}

// the listed groups at their compacted slots, keyed by their first item
__global__ __launch_bounds__(kBlock) void learn_first_keys_kernel(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                                                                  const uint32_t *__restrict__ group_first, size_t n_groups, size_t n_listed,
                                                                  uint64_t *__restrict__ key, uint32_t *__restrict__ listed_group) {
  const size_t g = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (g >= n_groups || !flag[g]) return;
  const uint32_t c = pos[g];
  if (!wp_in_bounds(c < n_listed, kSiteLearn)) return;
  listed_group[c] = static_cast<uint32_t>(g);
  key[c] = group_first[g];
}

// slot j of the order by first item: its group as the value and its score, descending, as the key of the second sort
__global__ __launch_bounds__(kBlock) void learn_score_keys_kernel(const uint32_t *__restrict__ val, const uint32_t *__restrict__ listed_group,
                                                                  const unsigned long long *__restrict__ sum, size_t n_listed, size_t n_groups,
                                                                  uint64_t *__restrict__ key, uint32_t *__restrict__ group) {
  const size_t j = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j >= n_listed) return;
  uint32_t g = 0;
  if (wp_in_bounds(val[j] < n_listed, kSiteLearn)) g = listed_group[val[j]];
  if (!wp_in_bounds(g < n_groups, kSiteLearn)) g = 0;
  group[j] = g;
  key[j] = ~static_cast<uint64_t>(sum[g]);  // (a kept score is at least the threshold: positive)
}

__device__ __forceinline__ uint32_t learn_cp_bytes(uint32_t cp) { return cp < 0x80u ? 1u : cp < 0x800u ? 2u : cp < 0x10000u ? 3u : 4u; }

// Entry t of the list: the reserved tokens, then every character bare and joined, then the listed groups in their
// order.  Per entry its score, where its text comes from (src, from), whether "##" goes in front, and its bytes with
// the '\n' behind it; len[n_entries] = 0 closes the lengths for their scan.
__global__ __launch_bounds__(kBlock) void learn_emit_kernel(const uint32_t *__restrict__ res_off, size_t n_res, const uint32_t *__restrict__ char_cp,
                                                            const int32_t *__restrict__ char_group, size_t n_chars,
                                                            const uint32_t *__restrict__ ordered_group, size_t n_listed,
                                                            const uint32_t *__restrict__ group_first, const uint32_t *__restrict__ item_word,
                                                            const uint16_t *__restrict__ item_se, const uint32_t *__restrict__ cell_off,
                                                            const uint32_t *__restrict__ cell, const uint32_t *__restrict__ kept,
                                                            const unsigned long long *__restrict__ sum, size_t n_groups, size_t n_items,
                                                            long long *__restrict__ scores, uint32_t *__restrict__ len, uint32_t *__restrict__ src,
                                                            uint8_t *__restrict__ from) {
  const size_t n_entries = n_res + 2 * n_chars + n_listed;
  const size_t t = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (t == 0) len[n_entries] = 0;
  if (t >= n_entries) return;
  long long score = 0;
  uint32_t bytes = 0, at = 0, how = kLearnFromReserved, joined = 0;
  if (t < n_res) {
    at = res_off[t];
    bytes = res_off[t + 1] - at;
  } else if (t < n_res + 2 * n_chars) {
    const size_t k = (t - n_res) >> 1;
    joined = static_cast<uint32_t>((t - n_res) & 1);
    at = char_cp[k];
    bytes = learn_cp_bytes(at);
    how = kLearnFromCp;
    const int32_t g = char_group[t - n_res];
    score = 1;
    if (g >= 0 && wp_in_bounds(static_cast<size_t>(g) < n_groups, kSiteLearn) && kept[g]) score = static_cast<long long>(sum[g]);
  } else {
    const uint32_t g = ordered_group[t - n_res - 2 * n_chars];
    how = kLearnFromPool;
    if (wp_in_bounds(g < n_groups && group_first[g] < n_items, kSiteLearn)) {
      const LearnSpan sp = learn_span(group_first[g], item_word, item_se, cell_off, cell);
      at = sp.a;
      bytes = sp.b - sp.a;
      joined = sp.joined;
      score = static_cast<long long>(sum[g]);
    }
  }
  scores[t] = score;
  len[t] = bytes + 2u * joined + 1u;
  src[t] = at;
  from[t] = static_cast<uint8_t>(how | (joined << 2));
}

// The text of the list, one byte per lane: the entry of byte p by bisection in token_off, then "##", the bytes of the
// reserved token, of the character or of the pool, and '\n' last.
__global__ __launch_bounds__(kBlock) void learn_gather_kernel(const uint8_t *__restrict__ pool, size_t pool_bytes, const uint8_t *__restrict__ res,
                                                              size_t res_bytes, const long long *__restrict__ token_off, const uint32_t *__restrict__ src,
                                                              const uint8_t *__restrict__ from, size_t n_entries, size_t cap,
                                                              uint8_t *__restrict__ out) {
  const size_t p = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (p >= cap || p >= static_cast<size_t>(token_off[n_entries])) return;  // (cap: the room of out, a bound the host knew before the scan)
  const size_t lo = last_le(token_off, size_t(0), n_entries, p);
  size_t k = p - static_cast<size_t>(token_off[lo]);
  const uint32_t how = from[lo] & 3u, joined = from[lo] >> 2;
  uint8_t b = 0;
  if (p + 1 == static_cast<size_t>(token_off[lo + 1])) {
    b = '\n';
  } else if (joined && k < 2) {
    b = '#';
  } else {
    k -= 2u * joined;
    const size_t at = static_cast<size_t>(src[lo]) + k;
    if (how == kLearnFromReserved) {
      b = wp_in_bounds(at < res_bytes, kSiteLearn) ? res[at] : 0;
    } else if (how == kLearnFromPool) {
      b = wp_in_bounds(at < pool_bytes, kSiteLearn) ? pool[at] : 0;
    } else {
      const uint32_t cp = src[lo], n = learn_cp_bytes(cp);
      const uint32_t shift = 6u * (n - 1u - static_cast<uint32_t>(k));
      if (n == 1) b = static_cast<uint8_t>(cp);
      else if (k == 0) b = static_cast<uint8_t>((0xf00u >> n & 0xf0u) | (cp >> shift));
      else b = static_cast<uint8_t>(0x80u | ((cp >> shift) & 0x3fu));
    }
  }
  out[p] = b;
}

}  // namespace wp
