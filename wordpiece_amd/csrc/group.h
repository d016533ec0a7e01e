// group.h — the device code that more than one grouping layer runs (host side: group_path.h; layers: count.h, learn.h,
// dedup.h, neardup.h, overlap.h and through it repeat.h): the 64-bit finaliser and the golden-ratio word of every key,
// the masked word loads and their comparison, the byte-absorbing hash loop, the one bisection, the run of a sorted
// position, the intake of a ragged batch's offsets, and the kernels of a grouping round, of the table and of the compact
// form.  Every kernel here counts a skipped access at kSiteGroup, whichever layer launched it, and the end check of
// every layer reads that site beside its own (group_path.h, throw_if_group_oob).  (group_starts_kernel is none of them:
// it belongs to the encode path, scanline.h: the slot starts of the walk's needed groups.)
#pragma once
#include "primitives.h"

namespace wp {

constexpr uint64_t kGolden = 0x9e3779b97f4a7c15ull;  // 2^64 / phi, odd: the word every seed and every hash step is offset by
constexpr uint32_t kNoBadRow = 0xffffffffu;          // the bad-row word while no row failed the offsets check

__device__ __forceinline__ uint64_t mix64(uint64_t h) {
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}

// h over the len bytes at p, 8 a step, the rest of them (or nothing) in a last step of its own
__device__ __forceinline__ uint64_t absorb_bytes(uint64_t h, const uint8_t *__restrict__ p, uint32_t len) {
  uint32_t i = 0;
  for (; i + 8 <= len; i += 8) {
    uint64_t x = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) x |= static_cast<uint64_t>(p[i + q]) << (8 * q);
    h = mix64(h ^ x) + kGolden;
  }
  uint64_t x = 0;
  for (int q = 0; i < len; i++, q++) x |= static_cast<uint64_t>(p[i]) << (8 * q);
  return mix64(h ^ x);
}

// The 4 bytes [s + 4 i, s + 4 i + 4) of the data as a little-endian word, zero from byte e on.  The loads are aligned
// words that begin below e: nothing behind the word that holds byte e - 1 is touched, and what that word holds behind
// e - 1 is masked away.
__device__ __forceinline__ uint32_t word_at(const uint32_t *__restrict__ d32, size_t s, size_t e, uint32_t i) {
  const size_t a = s + 4u * static_cast<size_t>(i);
  const size_t wi = a >> 2;
  const uint32_t sh = static_cast<uint32_t>(a & 3u) * 8u;
  uint32_t x = d32[wi] >> sh;
  if (sh != 0 && ((wi + 1) << 2) < e) x |= d32[wi + 1] << (32u - sh);
  const size_t rem = e - a;
  if (rem < 4) x &= (1u << (8u * static_cast<uint32_t>(rem))) - 1u;
  return x;
}

// whether the `bytes` bytes at a of data da equal those at b of data db; one lane reads them all
__device__ __forceinline__ bool same_words(const uint32_t *__restrict__ da, size_t a, const uint32_t *__restrict__ db, size_t b, uint32_t bytes) {
  const uint32_t words = (bytes + 3u) >> 2;
  for (uint32_t i = 0; i < words; i++) {
    if (word_at(da, a, a + bytes, i) != word_at(db, b, b + bytes, i)) return false;
  }
  return true;
}

// the last i in [lo, hi) with off[i] <= x, given off[lo] <= x (hi - lo shrinks on every step, whatever off holds: the loop ends).
// The indices are of the caller's width: 32 bits where they number rows (fewer than 2^31, so lo + hi does not wrap).
template <typename Off, typename Index>
__device__ __forceinline__ Index last_le(const Off *__restrict__ off, Index lo, Index hi, size_t x) {
  while (hi - lo > 1) {
    const Index mid = (lo + hi) >> 1;
    if (static_cast<size_t>(off[mid]) <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// the run of sorted position s (run: the exclusive scan of head, which counts the heads in front of s)
__device__ __forceinline__ uint32_t run_of(const uint32_t *__restrict__ head, const uint32_t *__restrict__ run, size_t s) {
  return run[s] + head[s] - 1u;
}

// Lane i <= n_rows of a layer's row kernel: byte_off[i] = the start of row i in bytes, and entry n_rows closes byte_off
// with the end of the data; that lane leaves row_off[n_rows] in *n_elems.  A row has its offsets checked (row_off[0] == 0,
// no descent; the smallest bad row wins).  The arithmetic is 64-bit and clamped: offsets that are wild give a bad row or
// a size the host refuses, never an index.
struct RaggedRow {
  bool row;                // false: the closing entry
  unsigned long long len;  // elements of the row, 0 where the offsets descend
};
__device__ __forceinline__ RaggedRow ragged_row(const long long *__restrict__ row_off, size_t n_rows, uint32_t elem_bytes, size_t i,
                                                uint32_t *__restrict__ byte_off, uint32_t *__restrict__ bad,
                                                unsigned long long *__restrict__ n_elems) {
  const long long a = row_off[i];
  const unsigned long long ab = static_cast<unsigned long long>(a) * elem_bytes;
  byte_off[i] = a < 0 || ab > 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(ab);
  if (i == n_rows) {
    *n_elems = static_cast<unsigned long long>(a);
    return RaggedRow{false, 0ull};
  }
  const long long b = row_off[i + 1];
  if (b < a || (i == 0 && a != 0)) atomicMin(bad, static_cast<uint32_t>(i));
  return RaggedRow{true, b < a ? 0ull : static_cast<unsigned long long>(b - a)};
}

// ---- a grouping round (group_path.h: group_runs, compact_flagged, carry_leftovers) -------------------------------------
// head[s] = 1 where sorted position s opens a run of equal keys
__global__ __launch_bounds__(kBlock) void group_heads_kernel(const uint64_t *__restrict__ key, size_t m, uint32_t *__restrict__ head) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s >= m) return;
  head[s] = (s == 0 || key[s] != key[s - 1]) ? 1u : 0u;
}

// head_pos[r] = the sorted position of the head of run r; head_pos[n_runs] = m (run: the exclusive scan of head)
__global__ __launch_bounds__(kBlock) void group_head_pos_kernel(const uint32_t *__restrict__ head, const uint32_t *__restrict__ run, size_t m,
                                                                const uint32_t *__restrict__ n_runs, uint32_t *__restrict__ head_pos) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s == 0 && wp_in_bounds(*n_runs <= m, kSiteGroup)) head_pos[*n_runs] = static_cast<uint32_t>(m);
  if (s >= m || !head[s]) return;
  if (wp_in_bounds(run[s] < m, kSiteGroup)) head_pos[run[s]] = static_cast<uint32_t>(s);
}

// out[pos[i]] = src ? src[i] : i wherever flag[i] (pos: the exclusive scan of flag)
__global__ __launch_bounds__(kBlock) void group_compact_kernel(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, size_t n,
                                                               const uint32_t *__restrict__ src, uint32_t *__restrict__ out, size_t cap) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n || !flag[i]) return;
  if (wp_in_bounds(pos[i] < cap, kSiteGroup)) out[pos[i]] = src ? src[i] : static_cast<uint32_t>(i);
}

// ---- the table and the compact form (group_path.h: group_table, compact_rows) -------------------------------------------
// keep[i] = 1 where row i is the first of its kind; entry n_rows closes the array for its scan
__global__ __launch_bounds__(kBlock) void group_keep_kernel(const int32_t *__restrict__ first, size_t n_rows, uint32_t *__restrict__ keep) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i > n_rows) return;
  keep[i] = i < n_rows && first[i] == static_cast<int32_t>(i) ? 1u : 0u;
}

// The table (keep_pos: the exclusive scan of keep): a kept row at its slot with its count and its length in bytes,
// every row with the slot of its first occurrence (inverse, optional).  out_len[n_unique] = 0 closes the lengths.
__global__ __launch_bounds__(kBlock) void group_table_kernel(const int32_t *__restrict__ first, const uint32_t *__restrict__ keep_pos,
                                                             const uint32_t *__restrict__ row_count, const uint32_t *__restrict__ byte_off,
                                                             size_t n_rows, size_t n_unique, int32_t *__restrict__ kept,
                                                             long long *__restrict__ counts, int32_t *__restrict__ inverse,
                                                             uint32_t *__restrict__ out_len) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i == 0 && out_len) out_len[n_unique] = 0;
  if (i >= n_rows) return;
  const int32_t f = first[i];
  if (!wp_checked(f >= 0 && static_cast<size_t>(f) <= i, kSiteGroup)) return;
  const uint32_t k = keep_pos[f];
  if (!wp_checked(k < n_unique, kSiteGroup)) return;
  if (inverse) inverse[i] = static_cast<int32_t>(k);
  if (static_cast<size_t>(f) == i) {
    kept[k] = static_cast<int32_t>(i);
    counts[k] = row_count[i];
    if (out_len) out_len[k] = byte_off[i + 1] - byte_off[i];
  }
}

// row_off[k] of the compact form, in elements (out_pos: the exclusive scan of out_len, in bytes); k in [0, n_unique]
__global__ __launch_bounds__(kBlock) void group_out_off_kernel(const uint32_t *__restrict__ out_pos, size_t n_unique, uint32_t elem_bytes,
                                                               long long *__restrict__ row_off) {
  const size_t k = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (k > n_unique) return;
  row_off[k] = static_cast<long long>(out_pos[k] / elem_bytes);
}

// The compact data, one lane per 4 output bytes: the kept row of the lane's first byte by bisection in out_pos
// (n_unique + 1 entries, in bytes), the rows of its other bytes by stepping on from there (rows of 1 to 3 bytes share a
// word; at most one kept row is empty), every byte from its place in the input.  The lanes run to the size the host
// knew before the scan (cap, the bytes of the input); *out_bytes ends them.
__global__ __launch_bounds__(kBlock) void group_gather_kernel(const uint8_t *__restrict__ data, size_t n_bytes, const uint32_t *__restrict__ byte_off,
                                                              const int32_t *__restrict__ kept, const uint32_t *__restrict__ out_pos,
                                                              size_t n_unique, size_t n_rows, size_t cap, uint32_t *__restrict__ out) {
  const size_t p = (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x) * 4u;
  const size_t total = out_pos[n_unique];
  if (p >= total || p >= cap) return;
  size_t lo = last_le(out_pos, size_t(0), n_unique, p);
  uint32_t w = 0;
  for (uint32_t b = 0; b < 4 && p + b < total; b++) {
    while (lo + 1 < n_unique && out_pos[lo + 1] <= p + b) lo++;
    const int32_t row = kept[lo];
    if (!wp_checked(row >= 0 && static_cast<size_t>(row) < n_rows, kSiteGroup)) continue;
    const size_t at = static_cast<size_t>(byte_off[row]) + (p + b - out_pos[lo]);
    if (wp_checked(at < n_bytes, kSiteGroup)) w |= static_cast<uint32_t>(data[at]) << (8u * b);
  }
  out[p >> 2] = w;
}

// off[t] = the bytes of the entries in front of t, each with `term` (0 or 1) terminator bytes; t in [0, n]
// (len_pos: the exclusive scan of the lengths)
__global__ __launch_bounds__(kBlock) void group_offsets_kernel(const uint32_t *__restrict__ len_pos, size_t n, int term, long long *__restrict__ off) {
  const size_t t = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (t > n) return;
  off[t] = static_cast<long long>(len_pos[t]) + static_cast<long long>(t) * term;
}

}  // namespace wp
