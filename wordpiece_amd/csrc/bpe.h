// bpe.h — kernels of the byte-level BPE encoder (include/wordpiece_amd_bpe.h; host path: bpe_path.h).
// Three stages:
//   1. class and start pass (bpe_start_kernel): a tile of kBpeTile bytes with a halo of 8 bytes on either side goes into LDS
//      once, as bytes, as break flags (first byte of a document, outside the text) and as one flag byte per byte: S, L, N,
//      U+0020, apostrophe, and the length of the character that starts there.  ASCII reads a 128-entry table and never the
//      paged one.  Rules 1-3 of the header are then local: a lane looks at most 7 flag bytes back and 3 ahead.  A ballot per
//      wave and trip is the start bitmap (one 64-bit word per 64 bytes), its population counts the tile's pieces; one scan
//      over the tiles and bpe_list_kernel give the piece list (start; the length is the distance to the next start).
//      Document starts are forced starts, so no piece spans two documents.
//   2. merge pass.  The pair table is open addressing in global memory, a 16-byte entry (left, right, rank, result) per
//      slot, at least twice as many slots as merges.  Pieces go one of three ways by their bytes:
//      - up to kBpeShort: one lane each (bpe_short_kernel), symbols, pair ranks and byte lengths in a private LDS strip,
//        lane-minor, so a wave's accesses never share a bank.  The ranks of the current pairs are kept: a merge costs the
//        two lookups beside the new symbol, not a rescan.
//      - up to kBpeMedium: one wave each (bpe_medium_kernel), everything in LDS, two strips that swap roles per round.
//      - longer: one workgroup each (bpe_long_kernel) over global scratch with the same loop, exact at any length; its
//        speed is not a goal.
//      The cooperative loop (bpe_merge_rounds) is one piece of code for both: the lowest rank by a reduction, every
//      occurrence merged in the same round — for a pair of two equal symbols every second one of a run, found by a max-scan
//      of the run starts — the survivors placed by a prefix sum, and only the pairs beside a new symbol looked up again.
//      A piece runs the loop once and writes its ids to provisional cells at its own byte offset (it never has more ids
//      than bytes) and its count.
//   3. compaction: a scan over the counts and one flat copy, a lane per byte (bpe_copy_kernel); row_splits, the offsets
//      and piece_splits come from the same scan.
// No atomic touches a result: the two atomics of the deal kernel feed statistics and a buffer size.
#pragma once
#include "../../include/wordpiece_amd_bpe.h"
#include "bpe_tables.h"
#include "classify.h"
#include "common.h"
#include "primitives.h"

namespace wp {

constexpr int kBpeItems = 4;                        // bytes per lane of a tile, one per trip
constexpr int kBpeTile = kBlock * kBpeItems;        // T: bytes per workgroup of the start pass
constexpr int kBpeHalo = 8;                         // bytes on either side: an apostrophe 3 back, its predecessor 4 further
constexpr int kBpeSpan = kBpeTile + 2 * kBpeHalo;   // flag bytes of a tile
constexpr int kBpeRaw = kBpeSpan + 4;               // text bytes of a tile: a character reads 3 bytes ahead
constexpr int kBpeGroups = kBpeTile / kWave;        // ballots per tile
constexpr int kBpeShort = 16;                       // bytes of a piece one lane merges
constexpr int kBpeMedium = 256;                     // bytes of a piece one wave merges in LDS
constexpr uint32_t kBpeNone = 0x7fffffffu;          // no rank (ranks stay below 2^30)
constexpr uint32_t kBpeEmpty = 0xffffffffu;         // the left id of an empty slot of the pair table
constexpr uint32_t kBpeS = 1, kBpeL = 2, kBpeN = 4, kBpeSp = 8, kBpeApos = 16, kBpeLenShift = 5;
static_assert(kBpeRaw % 4 == 0 && kBpeHalo % 4 == 0, "a tile is loaded in whole words");

// what a kernel knows of the model (device pointers)
struct BpeModel {
  const int32_t *byte_id, *merges;  // [256]; [n_merges][3]
  const uint4 *table;               // (left, right, rank, result)
  const uint16_t *cls_index;
  const uint8_t *cls_pages;
  uint32_t table_mask, n_merges, n_ids;
};

__host__ __device__ inline uint32_t bpe_pair_hash(uint32_t l, uint32_t r) {
  uint32_t h = l * 0x9E3779B1u ^ r * 0x85EBCA77u;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  return h ^ (h >> 13);
}

// the rank of the pair (l, r), or kBpeNone
__device__ __forceinline__ uint32_t bpe_lookup(const BpeModel &m, int32_t l, int32_t r) {
  uint32_t slot = bpe_pair_hash(static_cast<uint32_t>(l), static_cast<uint32_t>(r)) & m.table_mask;
  for (uint32_t tries = 0; tries <= m.table_mask; tries++, slot = (slot + 1) & m.table_mask) {
    const uint4 e = m.table[slot];
    if (e.x == kBpeEmpty) return kBpeNone;
    if (e.x == static_cast<uint32_t>(l) && e.y == static_cast<uint32_t>(r)) return e.z;
  }
  return kBpeNone;
}

__device__ __forceinline__ bool bpe_space_cp(uint32_t c) {
  return c == 0x85 || c == 0xa0 || c == 0x1680 || (c >= 0x2000 && c <= 0x200a) || c == 0x2028 || c == 0x2029 || c == 0x202f || c == 0x205f || c == 0x3000;
}

// ---- 1. the class and start pass -------------------------------------------------------------------------------------------
// The flag byte of span position i: sb, the text bytes from there on; brk, the break flags.  A sequence that a document
// start or the end of the text cuts is not well formed: its bytes are characters of class O, one each.
__device__ __forceinline__ uint32_t bpe_class(const uint8_t *sb, const uint8_t *brk, int i, const BpeModel &m) {
  if ((brk[i] & 2u) != 0) return 0u;
  const uint32_t b0 = sb[i];
  if (b0 < 0x80u) return kBpeAscii[b0];
  int room = 1;
  while (room < 4 && brk[i + room] == 0) room++;
  const uint32_t cp = decode_one(sb + i, room);
  if (cp == kInvalidUnicode) return 1u << kBpeLenShift;
  const uint32_t len = cp < 0x800u ? 2u : cp < 0x10000u ? 3u : 4u;
  uint32_t c = len << kBpeLenShift;
  if (bpe_space_cp(cp)) return c | kBpeS;
  const uint32_t k = m.cls_pages[static_cast<uint32_t>(m.cls_index[cp >> 8]) * 256u + (cp & 255u)];
  return c | ((k & 1u) ? kBpeL : 0u) | ((k & 2u) ? kBpeN : 0u);
}

// the tile's text, break flags and flag bytes, and the rules over them (i: a span position, kBpeHalo + the byte in the tile)
struct BpeTile {
  const uint8_t *sb, *brk, *cls;
  __device__ __forceinline__ uint32_t len(int i) const { return cls[i] >> kBpeLenShift; }
  // the start of the character in front of the character start i (i starts no document)
  __device__ __forceinline__ int pred(int i) const {
    for (int k = 2; k <= 4; k++) {
      if (len(i - k) == static_cast<uint32_t>(k)) return i - k;
    }
    return i - 1;
  }
  // rule 2 for the character start i, which is not S
  __device__ __forceinline__ bool rule2(int i) const {
    if (brk[i] != 0) return true;
    const uint32_t pc = cls[pred(i)];
    if ((pc & kBpeS) != 0) return (pc & kBpeSp) == 0;
    return (pc & (kBpeL | kBpeN)) != (cls[i] & (kBpeL | kBpeN));
  }
  // the bytes of the contraction whose apostrophe is span position a: 2, 3, or 0 where there is none
  __device__ __forceinline__ int contraction(int a) const {
    if ((cls[a] & kBpeApos) == 0 || brk[a + 1] != 0 || !rule2(a)) return 0;
    const uint32_t b1 = sb[a + 1];
    if (b1 == 's' || b1 == 't' || b1 == 'm' || b1 == 'd') return 2;
    if (brk[a + 2] != 0) return 0;
    const uint32_t b2 = sb[a + 2];
    return ((b1 == 'r' && b2 == 'e') || (b1 == 'v' && b2 == 'e') || (b1 == 'l' && b2 == 'l')) ? 3 : 0;
  }
  // whether a piece starts at span position i of the tile proper
  __device__ __forceinline__ bool start(int i) const {
    const uint32_t c = cls[i];
    if (c == 0) return false;  // outside the text
    for (int k = 1; k <= 3; k++) {
      if (len(i - k) > static_cast<uint32_t>(k)) return false;  // a later byte of a character
    }
    if (brk[i] != 0) return true;  // the first character of a document
    if ((c & kBpeS) != 0) {
      if ((cls[pred(i)] & kBpeS) == 0) return true;
      const int nxt = i + static_cast<int>(len(i));
      return brk[nxt] == 0 && (cls[nxt] & kBpeS) == 0;
    }
    if (contraction(i - 1) != 0) return false;
    const int k2 = contraction(i - 2);
    if (k2 != 0) return k2 == 2;
    if (contraction(i - 3) == 3) return true;
    return rule2(i);
  }
};

// startbits[p / 64]: the ballot of the starts among bytes [p, p + 64); tiles[t]: the starts of tile t
__global__ __launch_bounds__(kBlock) void bpe_start_kernel(const uint32_t *__restrict__ text32, size_t nb, const uint32_t *__restrict__ docbits, BpeModel m,
                                                           unsigned long long *__restrict__ startbits, uint32_t *__restrict__ tiles) {
  __shared__ uint32_t sw[kBpeRaw / 4];
  __shared__ uint8_t brk[kBpeRaw], cls[kBpeSpan];
  __shared__ uint32_t s_cnt[kBlock / kWave];
  const long long base = static_cast<long long>(blockIdx.x) * kBpeTile, lo = base - kBpeHalo, n = static_cast<long long>(nb);
  for (int i = threadIdx.x; i < kBpeRaw / 4; i += kBlock) {
    const long long p = lo + 4ll * i;
    sw[i] = (p >= 0 && p < n) ? text32[p >> 2] : 0u;
  }
  for (int i = threadIdx.x; i < kBpeRaw; i += kBlock) {
    const long long p = lo + i;
    brk[i] = (p < 0 || p >= n) ? 2u : static_cast<uint8_t>((docbits[p >> 5] >> (p & 31)) & 1u);
  }
  __syncthreads();
  const uint8_t *sb = reinterpret_cast<const uint8_t *>(sw);
  for (int i = threadIdx.x; i < kBpeSpan; i += kBlock) cls[i] = static_cast<uint8_t>(bpe_class(sb, brk, i, m));
  __syncthreads();
  const BpeTile t{sb, brk, cls};
  uint32_t count = 0;
  for (int it = 0; it < kBpeItems; it++) {
    const int at = it * kBlock + threadIdx.x;
    const unsigned long long ballot = __ballot(t.start(kBpeHalo + at) ? 1 : 0);
    if (lane_id() == 0) startbits[(base + at) >> 6] = ballot;
    count += static_cast<uint32_t>(__popcll(ballot));
  }
  if (lane_id() == 0) s_cnt[wave_id()] = count;
  __syncthreads();
  if (threadIdx.x == 0) tiles[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// the ballots of tile `tile` into s_mask and the starts in front of each into s_pre (kBpeGroups entries each)
__device__ __forceinline__ void bpe_tile_prefix(const unsigned long long *__restrict__ startbits, size_t tile, unsigned long long *s_mask, uint32_t *s_pre) {
  if (threadIdx.x < kBpeGroups) s_mask[threadIdx.x] = startbits[tile * kBpeGroups + threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t a = 0;
    for (int g = 0; g < kBpeGroups; g++) {
      s_pre[g] = a;
      a += static_cast<uint32_t>(__popcll(s_mask[g]));
    }
  }
  __syncthreads();
}

// tiles holds the scan; pstart[k]: the first byte of piece k, pstart[n_pieces] = nb
__global__ __launch_bounds__(kBlock) void bpe_list_kernel(const unsigned long long *__restrict__ startbits, const uint32_t *__restrict__ tiles, size_t nb,
                                                          size_t n_pieces, uint32_t *__restrict__ pstart) {
  __shared__ unsigned long long s_mask[kBpeGroups];
  __shared__ uint32_t s_pre[kBpeGroups];
  bpe_tile_prefix(startbits, blockIdx.x, s_mask, s_pre);
  const int lane = lane_id();
  for (int it = 0; it < kBpeItems; it++) {
    const int g = it * (kBlock / kWave) + wave_id();
    const unsigned long long mask = s_mask[g];
    if (((mask >> lane) & 1ull) == 0) continue;
    const size_t k = static_cast<size_t>(tiles[blockIdx.x]) + s_pre[g] + static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)));
    if (wp_checked(k < n_pieces, kSiteQuality)) pstart[k] = static_cast<uint32_t>(static_cast<size_t>(blockIdx.x) * kBpeTile + g * kWave + lane);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) pstart[n_pieces] = static_cast<uint32_t>(nb);
}

// the pieces dealt to their paths: med[k], lng[k] the flags of the medium and long ones (entry n_pieces closes each for its
// scan); stats: the longest piece (64 bits) and behind it the bytes of the long pieces (the size of their scratch)
__global__ __launch_bounds__(kBlock) void bpe_deal_kernel(const uint32_t *__restrict__ pstart, size_t n_pieces, uint32_t *__restrict__ med, uint32_t *__restrict__ lng,
                                                          unsigned long long *__restrict__ longest, uint32_t *__restrict__ long_bytes) {
  const size_t k = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  uint32_t len = 0;
  if (k < n_pieces) len = pstart[k + 1] - pstart[k];
  if (k <= n_pieces) {
    med[k] = (len > kBpeShort && len <= kBpeMedium) ? 1u : 0u;
    lng[k] = len > kBpeMedium ? 1u : 0u;
  }
  if (len > kBpeMedium) atomicAdd(long_bytes, len);
  const uint32_t top = static_cast<uint32_t>(-wave_reduce_min(-static_cast<int32_t>(min(len, 0x7fffffffu))));
  if (lane_id() == 0 && top != 0) atomicMax(longest, static_cast<unsigned long long>(top));
}

// the lists of the medium and the long pieces from the scans of their flags; llen: the bytes of each long piece
__global__ __launch_bounds__(kBlock) void bpe_lists_kernel(const uint32_t *__restrict__ pstart, size_t n_pieces, const uint32_t *__restrict__ med,
                                                           const uint32_t *__restrict__ med_pos, size_t n_med, const uint32_t *__restrict__ lng,
                                                           const uint32_t *__restrict__ lng_pos, size_t n_lng, uint32_t *__restrict__ mlist, uint32_t *__restrict__ llist,
                                                           uint32_t *__restrict__ llen) {
  const size_t k = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (k >= n_pieces) return;
  if (med[k] && wp_checked(med_pos[k] < n_med, kSiteQuality)) mlist[med_pos[k]] = static_cast<uint32_t>(k);
  if (lng[k] && wp_checked(lng_pos[k] < n_lng, kSiteQuality)) {
    llist[lng_pos[k]] = static_cast<uint32_t>(k);
    llen[lng_pos[k]] = pstart[k + 1] - pstart[k];
  }
  if (k == 0) llen[n_lng] = 0;
}

// ---- 2. the merge pass -------------------------------------------------------------------------------------------------------
// what the provisional cells of a call are: ids and, with offsets, the end of every id in bytes from the piece's start,
// both at the piece's own byte offset; cnt[k]: the ids of piece k
struct BpeCells {
  int32_t *ids;
  uint32_t *ends;  // nullptr: no offsets
  uint32_t *cnt;
};

// one lane per piece of at most kBpeShort bytes
__global__ __launch_bounds__(kBlock) void bpe_short_kernel(const uint8_t *__restrict__ text, size_t nb, const uint32_t *__restrict__ pstart, size_t n_pieces, BpeModel m,
                                                           BpeCells out) {
  __shared__ int32_t s_sym[kBpeShort][kBlock];
  __shared__ uint32_t s_rk[kBpeShort][kBlock];
  __shared__ uint8_t s_len[kBpeShort][kBlock];
  const size_t k = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (k >= n_pieces) return;
  const uint32_t s = pstart[k], e = pstart[k + 1];
  if (e - s > kBpeShort || !wp_checked(s < e && e <= nb, kSiteQuality)) return;
  const int t = threadIdx.x;
  int n = static_cast<int>(e - s);
  for (int i = 0; i < n; i++) {
    s_sym[i][t] = m.byte_id[text[s + i]];
    s_len[i][t] = 1;
  }
  for (int i = 0; i < n; i++) s_rk[i][t] = i + 1 < n ? bpe_lookup(m, s_sym[i][t], s_sym[i + 1][t]) : kBpeNone;
  while (n > 1) {
    uint32_t best = kBpeNone;
    for (int i = 0; i + 1 < n; i++) best = min(best, s_rk[i][t]);
    if (best >= m.n_merges) break;
    const int32_t result = m.merges[3 * static_cast<size_t>(best) + 2];
    // left to right: source i (merged with i + 1 where their pair has the rank) becomes output w <= i.  s_rk[w - 1] is
    // looked up where either side is new, and else is the rank the two sources had, carried when output w - 1 was written.
    int w = 0;
    bool prev_new = false;
    for (int i = 0; i < n; w++) {
      const uint32_t r = s_rk[i][t];
      const bool take = r == best;  // (the last rank is kBpeNone: i + 1 < n here)
      const int32_t sym = take ? result : s_sym[i][t];
      const uint32_t len = take ? static_cast<uint32_t>(s_len[i][t]) + s_len[i + 1][t] : s_len[i][t];
      if (w > 0 && (prev_new || take)) s_rk[w - 1][t] = bpe_lookup(m, s_sym[w - 1][t], sym);
      s_sym[w][t] = sym;
      s_len[w][t] = static_cast<uint8_t>(len);
      i += take ? 2 : 1;
      s_rk[w][t] = (take || i >= n) ? kBpeNone : r;
      prev_new = take;
    }
    n = w;
  }
  uint32_t end = 0;
  for (int j = 0; j < n; j++) {
    out.ids[s + j] = s_sym[j][t];
    end += s_len[j][t];
    if (out.ends) out.ends[s + j] = end;
  }
  out.cnt[k] = static_cast<uint32_t>(n);
}

// The lanes that merge one piece together: a wave over LDS, or a workgroup over global memory.
struct BpeWave {
  static constexpr int kSize = kWave;
  __device__ __forceinline__ int tid() const { return lane_id(); }
  __device__ __forceinline__ void sync() const {
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
  }
  __device__ __forceinline__ uint32_t reduce_min(uint32_t v) const { return static_cast<uint32_t>(wave_reduce_min(static_cast<int32_t>(v))); }
  __device__ __forceinline__ uint32_t excl_sum(uint32_t v, uint32_t &total) const {
    const uint32_t inc = wave_incl_sum(v);
    total = __shfl(inc, kWave - 1, kWave);
    return inc - v;
  }
  __device__ __forceinline__ int32_t incl_max(int32_t v) const { return wave_incl_max(v); }
};
struct BpeBlock {
  static constexpr int kSize = kBlock;
  uint32_t *smem;  // 8 words of LDS
  __device__ __forceinline__ int tid() const { return threadIdx.x; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  __device__ __forceinline__ uint32_t reduce_min(uint32_t v) const { return static_cast<uint32_t>(block_reduce_min(static_cast<int32_t>(v), reinterpret_cast<int32_t *>(smem))); }
  __device__ __forceinline__ uint32_t excl_sum(uint32_t v, uint32_t &total) const { return block_excl_sum(v, smem, total); }
  __device__ __forceinline__ int32_t incl_max(int32_t v) const { return block_incl_max(v, reinterpret_cast<int32_t *>(smem)); }
};

// one strip of a cooperative merge: symbols, the rank of the pair each forms with the next (kBpeNone behind the last), bytes
struct BpeStrip {
  int32_t *sym;
  uint32_t *rk, *len;
};

// The rounds of one piece whose n byte ids and lengths stand in a (header: "Merge").  a and b swap roles per round; fresh:
// n flags.  Returns the ids left, *out the strip they stand in.  Every lane of the group runs the same trips.
template <typename G>
__device__ size_t bpe_merge_rounds(const G &g, const BpeModel &m, BpeStrip a, BpeStrip b, uint8_t *fresh, size_t n, BpeStrip *out) {
  const size_t t = static_cast<size_t>(g.tid());
  for (size_t i = t; i < n; i += G::kSize) a.rk[i] = i + 1 < n ? bpe_lookup(m, a.sym[i], a.sym[i + 1]) : kBpeNone;
  g.sync();
  for (;;) {
    uint32_t best = kBpeNone;
    for (size_t i = t; i < n; i += G::kSize) best = min(best, a.rk[i]);
    best = g.reduce_min(best);
    if (best >= m.n_merges) break;
    const int32_t left = m.merges[3 * static_cast<size_t>(best)], right = m.merges[3 * static_cast<size_t>(best) + 1], result = m.merges[3 * static_cast<size_t>(best) + 2];
    const bool twin = left == right;
    size_t placed = 0;
    uint32_t run_odd = 0;  // twin: the parity of the run of `left` that reaches the end of the chunks so far
    for (size_t base = 0; base < n; base += G::kSize) {
      const size_t i = base + t;
      const bool in = i < n;
      const int32_t sym = in ? a.sym[i] : -1;
      const uint32_t r = in ? a.rk[i] : kBpeNone;
      bool take = r == best, prev_take = in && i > 0 && a.rk[i - 1] == best;
      if (twin) {
        // of a run of `left` every second pair merges, from the run's start on: the offset of i in its run, from the last
        // run start of the chunk at or in front of i, or from the parity the chunks in front leave
        const bool here = in && sym == left, before = in && i > 0 && a.sym[i - 1] == left;
        const int32_t rs = g.incl_max(here && !before ? static_cast<int32_t>(t) : -1);
        const uint32_t offset = rs >= 0 ? static_cast<uint32_t>(t) - static_cast<uint32_t>(rs) : static_cast<uint32_t>(t) + run_odd;
        take = take && (offset & 1u) == 0;
        prev_take = prev_take && (offset & 1u) == 1;
        // (the same for every lane: the chunk's last symbol and the last run start in front of it)
        const size_t last = base + G::kSize - 1;
        if (last < n && a.sym[last] == left) {
          size_t q = last;
          while (q > base && a.sym[q - 1] == left) q--;
          run_odd = (q == base && base > 0 && a.sym[base - 1] == left) ? run_odd : static_cast<uint32_t>((last - q + 1) & 1u);
        } else {
          run_odd = 0;
        }
      }
      const bool keep = in && !prev_take;
      uint32_t total;
      const size_t w = placed + g.excl_sum(keep ? 1u : 0u, total);
      if (keep) {
        b.sym[w] = take ? result : sym;
        b.len[w] = take ? a.len[i] + a.len[i + 1] : a.len[i];
        b.rk[w] = take ? kBpeNone : r;  // (carried: right where neither this symbol nor the next is new)
        fresh[w] = take ? 1 : 0;
      }
      placed += total;
    }
    g.sync();
    for (size_t w = t; w < placed; w += G::kSize) {
      if (w + 1 >= placed) {
        b.rk[w] = kBpeNone;
      } else if (fresh[w] || fresh[w + 1]) {
        b.rk[w] = bpe_lookup(m, b.sym[w], b.sym[w + 1]);
      }
    }
    g.sync();
    const BpeStrip s = a;
    a = b;
    b = s;
    n = placed;
  }
  *out = a;
  return n;
}

// the byte ids of piece [s, s + n) into strip a
template <typename G>
__device__ __forceinline__ void bpe_load_piece(const G &g, const BpeModel &m, const uint8_t *__restrict__ text, uint32_t s, size_t n, BpeStrip a) {
  for (size_t i = g.tid(); i < n; i += G::kSize) {
    a.sym[i] = m.byte_id[text[s + i]];
    a.len[i] = 1;
  }
  g.sync();
}

// the n ids of piece k, which starts at byte s, from strip a to their provisional cells
template <typename G>
__device__ __forceinline__ void bpe_store_piece(const G &g, BpeStrip a, size_t n, uint32_t s, size_t k, BpeCells out) {
  const size_t t = static_cast<size_t>(g.tid());
  for (size_t i = t; i < n; i += G::kSize) out.ids[s + i] = a.sym[i];
  if (out.ends) {
    uint32_t carry = 0;
    for (size_t base = 0; base < n; base += G::kSize) {
      const size_t i = base + t;
      const uint32_t v = i < n ? a.len[i] : 0u;
      uint32_t total;
      const uint32_t ex = g.excl_sum(v, total);
      if (i < n) out.ends[s + i] = carry + ex + v;
      carry += total;
    }
  }
  if (t == 0) out.cnt[k] = static_cast<uint32_t>(n);
}

// one wave per piece of list (pieces of kBpeShort + 1 .. kBpeMedium bytes)
__global__ __launch_bounds__(kBlock) void bpe_medium_kernel(const uint8_t *__restrict__ text, size_t nb, const uint32_t *__restrict__ pstart, size_t n_pieces,
                                                            const uint32_t *__restrict__ list, size_t n_list, BpeModel m, BpeCells out) {
  __shared__ int32_t s_sym[2][kBlock / kWave][kBpeMedium];
  __shared__ uint32_t s_rk[2][kBlock / kWave][kBpeMedium], s_len[2][kBlock / kWave][kBpeMedium];
  __shared__ uint8_t s_fresh[kBlock / kWave][kBpeMedium];
  const int w = wave_id();
  const size_t j = static_cast<size_t>(blockIdx.x) * (kBlock / kWave) + w;
  if (j >= n_list) return;
  const size_t k = list[j];
  if (!wp_checked(k < n_pieces, kSiteQuality)) return;
  const uint32_t s = pstart[k], e = pstart[k + 1];
  if (!wp_checked(s < e && e <= nb && e - s <= kBpeMedium, kSiteQuality)) return;
  const BpeWave g;
  BpeStrip a{s_sym[0][w], s_rk[0][w], s_len[0][w]}, b{s_sym[1][w], s_rk[1][w], s_len[1][w]}, last;
  bpe_load_piece(g, m, text, s, e - s, a);
  const size_t n = bpe_merge_rounds(g, m, a, b, s_fresh[w], e - s, &last);
  bpe_store_piece(g, last, n, s, k, out);
}

// One workgroup per piece of list (pieces of more than kBpeMedium bytes), over global scratch: piece j owns [loff[j],
// loff[j + 1]) of each of the seven arrays, scr_* holding 2 * room entries (the two strips) and fresh room bytes.
__global__ __launch_bounds__(kBlock) void bpe_long_kernel(const uint8_t *__restrict__ text, size_t nb, const uint32_t *__restrict__ pstart, size_t n_pieces,
                                                          const uint32_t *__restrict__ list, const uint32_t *__restrict__ loff, size_t n_list, size_t room, BpeModel m,
                                                          int32_t *scr_sym, uint32_t *scr_rk, uint32_t *scr_len, uint8_t *fresh, BpeCells out) {
  __shared__ uint32_t smem[8];
  const size_t j = blockIdx.x;
  if (j >= n_list) return;
  const size_t k = list[j], o = loff[j];
  if (!wp_checked(k < n_pieces, kSiteQuality)) return;
  const uint32_t s = pstart[k], e = pstart[k + 1];
  if (!wp_checked(s < e && e <= nb && o + (e - s) <= room && loff[j + 1] - o == e - s, kSiteQuality)) return;
  const BpeBlock g{smem};
  BpeStrip a{scr_sym + o, scr_rk + o, scr_len + o}, b{scr_sym + room + o, scr_rk + room + o, scr_len + room + o}, last;
  bpe_load_piece(g, m, text, s, e - s, a);
  const size_t n = bpe_merge_rounds(g, m, a, b, fresh + o, e - s, &last);
  bpe_store_piece(g, last, n, s, k, out);
}

// ---- 3. the compaction ---------------------------------------------------------------------------------------------------------
// what a call hands out (begin, end, piece_splits: nullptr unless asked for)
struct BpeOut {
  int32_t *ids, *begin, *end;
  long long *row_splits, *piece_splits;
};

// the pieces that start in front of byte b <= nb
__device__ __forceinline__ size_t bpe_pieces_before(const unsigned long long *__restrict__ startbits, const uint32_t *__restrict__ tiles, size_t nb, size_t n_pieces,
                                                    size_t b) {
  if (b >= nb) return n_pieces;
  const size_t tile = b / kBpeTile, g = (b % kBpeTile) / kWave;
  size_t k = tiles[tile];
  for (size_t q = 0; q < g; q++) k += static_cast<size_t>(__popcll(startbits[tile * kBpeGroups + q]));
  return min(n_pieces, k + static_cast<size_t>(__popcll(startbits[tile * kBpeGroups + g] & ((1ull << (b & 63)) - 1ull))));
}

// One lane per byte p: the piece k that holds it, and where p - pstart[k] is below the piece's count, the id in the
// provisional cell p to its place idpos[k] + (p - pstart[k]), with its bytes as offsets into the document.
__global__ __launch_bounds__(kBlock) void bpe_copy_kernel(const unsigned long long *__restrict__ startbits, const uint32_t *__restrict__ tiles, size_t nb,
                                                          const uint32_t *__restrict__ pstart, const uint32_t *__restrict__ idpos, size_t n_pieces, BpeCells cells,
                                                          const uint32_t *__restrict__ boff, size_t n_rows, size_t n_out, BpeOut out) {
  __shared__ unsigned long long s_mask[kBpeGroups];
  __shared__ uint32_t s_pre[kBpeGroups];
  bpe_tile_prefix(startbits, blockIdx.x, s_mask, s_pre);
  const int lane = lane_id();
  for (int it = 0; it < kBpeItems; it++) {
    const int g = it * (kBlock / kWave) + wave_id();
    const size_t p = static_cast<size_t>(blockIdx.x) * kBpeTile + g * kWave + lane;
    if (p >= nb) continue;
    const size_t upto = static_cast<size_t>(tiles[blockIdx.x]) + s_pre[g] + static_cast<uint32_t>(__popcll(s_mask[g] & bits_up_to(lane)));
    if (!wp_checked(upto >= 1 && upto <= n_pieces, kSiteQuality)) continue;
    const size_t k = upto - 1;
    const uint32_t s = pstart[k];
    if (!wp_checked(s <= p, kSiteQuality)) continue;
    const size_t j = p - s;
    if (j >= cells.cnt[k]) continue;
    const size_t at = static_cast<size_t>(idpos[k]) + j;
    if (!wp_checked(at < n_out, kSiteQuality)) continue;
    out.ids[at] = cells.ids[p];
    if (out.begin) {
      const uint32_t doc = boff[cls_row_of(boff, n_rows, static_cast<uint32_t>(p))];
      out.begin[at] = static_cast<int32_t>(s - doc + (j ? cells.ends[p - 1] : 0u));
      out.end[at] = static_cast<int32_t>(s - doc + cells.ends[p]);
    }
  }
}

// row_splits[r], r <= n_rows: the ids in front of document r; piece_splits[k], k <= n_pieces: those in front of piece k
__global__ __launch_bounds__(kBlock) void bpe_splits_kernel(const unsigned long long *__restrict__ startbits, const uint32_t *__restrict__ tiles, size_t nb,
                                                            const uint32_t *__restrict__ idpos, size_t n_pieces, const uint32_t *__restrict__ boff, size_t n_rows,
                                                            BpeOut out) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i <= n_rows) out.row_splits[i] = idpos[bpe_pieces_before(startbits, tiles, nb, n_pieces, boff[i])];
  if (out.piece_splits && i <= n_pieces) out.piece_splits[i] = idpos[i];
}

}  // namespace wp
