// special.h — special-token literals in the text of an encode (wp_linear_encode_special / _rows): the kernels.
//
// A listed vocabulary line "[...]" that stands in the text keeps its id.  The literals are found in the caller's text
// (match), overwritten with blanks in a copy that the encoder then sees (blank), given their place among the ids of
// that encode (place) and merged into its result (merge).  A literal is decided by the text alone: at a '[' the bytes
// up to and including the next ']' — at most kSpecialMaxLine of them, all in 0x21..0x7E, no further '[' — either equal
// a listed line or do not, so every '[' is looked at on its own and two literals never overlap.
#pragma once
#include "../../include/wordpiece_amd.h"
#include "decode.h"
#include "primitives.h"

namespace wp {

constexpr int kSpecialMaxLine = 64;    // bytes of a line that may be listed (a row of the table)
constexpr int kSpecialMaxListed = 4096;
constexpr int kSpecialIters = 4;
constexpr int kSpecialTile = kBlock * kDecChunk * kSpecialIters;  // 16 KB of text per workgroup
constexpr int kSpecialMergeItems = 8;
constexpr int kSpecialMergeTile = kBlock * kSpecialMergeItems;    // output cells per workgroup of the merge

// The listed lines on the device: n rows of kSpecialMaxLine bytes, zero behind the line, in ascending byte order (a
// line holds no zero byte, so the padded rows order the lines); ids[k] = the id of row k.
struct SpecialTable {
  const uint8_t *lines;
  const int32_t *ids;
  int n;
};

// Which of the 16 bytes at `off` are '[' (bit j: byte off + j), inside the text only.  text: 4-byte aligned and
// readable up to the next multiple of 16 behind nbytes; off: a multiple of 16.
__device__ __forceinline__ uint32_t special_brackets16(const uint8_t *__restrict__ text, size_t nbytes, size_t off) {
  if (off >= nbytes) return 0u;
  const dec_u32x4 v = *reinterpret_cast<const dec_u32x4 *>(text + off);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t x = w[k] ^ 0x5b5b5b5bu;  // a zero byte where the text has '['
    const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & kHi;
    m |= byte_mask4(z) << (4 * k);
  }
  return m & dec_inside16(off, nbytes);  // (the tail behind nbytes is padding, whatever it holds)
}

// The literal that starts at the '[' at byte p: its row in the table (and its length in *len), or -1.  Reads text
// bytes below nbytes only: a candidate that the end of the text cuts is none.
__device__ __forceinline__ int special_match_at(const uint8_t *__restrict__ text, size_t nbytes, size_t p, const SpecialTable &t,
                                                uint32_t *len) {
  uint32_t l = 1;
  for (;; l++) {
    if (l >= static_cast<uint32_t>(kSpecialMaxLine) || p + l >= nbytes) return -1;
    const uint32_t b = text[p + l];
    if (b == 0x5du) break;
    if (b < 0x21u || b > 0x7eu || b == 0x5bu) return -1;
  }
  l++;  // (the ']')
  int lo = 0, hi = t.n;  // first row >= the candidate
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    const uint8_t *row = t.lines + static_cast<size_t>(mid) * kSpecialMaxLine;
    int cmp = 0;  // row against candidate, both zero behind their ends
    for (uint32_t k = 0; k < static_cast<uint32_t>(kSpecialMaxLine) && cmp == 0; k++) {
      const int a = row[k], b = k < l ? text[p + k] : 0;
      cmp = a - b;
      if (a == 0 && b == 0) break;
    }
    if (cmp < 0) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  if (lo >= t.n) return -1;
  const uint8_t *row = t.lines + static_cast<size_t>(lo) * kSpecialMaxLine;
  for (uint32_t k = 0; k < l; k++) {
    if (row[k] != text[p + k]) return -1;
  }
  if (l < static_cast<uint32_t>(kSpecialMaxLine) && row[l] != 0) return -1;
  *len = l;
  return lo;
}

// match, pass 1: literals per tile.  A lane whose 16 bytes hold no '[' is done with them after one word-wide test.
__global__ __launch_bounds__(kBlock) void special_count_kernel(const uint8_t *__restrict__ text, size_t nbytes, SpecialTable tab,
                                                               uint32_t *__restrict__ tile_cnt) {
  __shared__ uint32_t sm[8];
  const size_t tile_base = static_cast<size_t>(blockIdx.x) * kSpecialTile;
  uint32_t m[kSpecialIters];
#pragma unroll
  for (int j = 0; j < kSpecialIters; j++) {
    m[j] = special_brackets16(text, nbytes, tile_base + (static_cast<size_t>(j) * kBlock + threadIdx.x) * kDecChunk);
  }
  uint32_t cnt = 0;
#pragma unroll
  for (int j = 0; j < kSpecialIters; j++) {
    const size_t off = tile_base + (static_cast<size_t>(j) * kBlock + threadIdx.x) * kDecChunk;
    uint32_t mm = m[j];
    while (mm) {
      const int b = __ffs(static_cast<int>(mm)) - 1;
      mm &= mm - 1u;
      uint32_t len;
      if (special_match_at(text, nbytes, off + static_cast<size_t>(b), tab, &len) >= 0) cnt++;
    }
  }
  uint32_t total;
  (void)block_excl_sum(cnt, sm, total);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// match, pass 2: the literals in text order (tile_prefix: the exclusive scan of pass 1): byte start, length, id
__global__ __launch_bounds__(kBlock) void special_write_kernel(const uint8_t *__restrict__ text, size_t nbytes, SpecialTable tab,
                                                               const uint32_t *__restrict__ tile_prefix, uint32_t n_lits,
                                                               uint32_t *__restrict__ lit_start, uint32_t *__restrict__ lit_len,
                                                               int32_t *__restrict__ lit_id) {
  __shared__ uint32_t sm[8];
  const size_t tile_base = static_cast<size_t>(blockIdx.x) * kSpecialTile;
  uint32_t carry = tile_prefix[blockIdx.x];
  uint32_t m[kSpecialIters];
#pragma unroll
  for (int j = 0; j < kSpecialIters; j++) {
    m[j] = special_brackets16(text, nbytes, tile_base + (static_cast<size_t>(j) * kBlock + threadIdx.x) * kDecChunk);
  }
#pragma unroll
  for (int j = 0; j < kSpecialIters; j++) {
    if (!__syncthreads_or(m[j] != 0u)) continue;  // (block-uniform)
    const size_t off = tile_base + (static_cast<size_t>(j) * kBlock + threadIdx.x) * kDecChunk;
    uint32_t hit = 0, mm = m[j];
    while (mm) {
      const int b = __ffs(static_cast<int>(mm)) - 1;
      mm &= mm - 1u;
      uint32_t len;
      if (special_match_at(text, nbytes, off + static_cast<size_t>(b), tab, &len) >= 0) hit |= 1u << b;
    }
    uint32_t total;
    uint32_t o = carry + block_excl_sum(__popc(hit), sm, total);
    while (hit) {
      const int b = __ffs(static_cast<int>(hit)) - 1;
      hit &= hit - 1u;
      uint32_t len = 0;
      const int row = special_match_at(text, nbytes, off + static_cast<size_t>(b), tab, &len);
      const bool ok = row >= 0 && o < n_lits;
      if (wp_in_bounds(ok, kSiteSpecial) && ok) {
        lit_start[o] = static_cast<uint32_t>(off) + static_cast<uint32_t>(b);
        lit_len[o] = len;
        lit_id[o] = tab.ids[row];
      }
      o++;
    }
    carry += total;
  }
}

// blank: 0x20 over every literal of the copy (a literal's bytes are its own: no two threads store to one byte)
__global__ __launch_bounds__(kBlock) void special_blank_kernel(uint8_t *__restrict__ copy, size_t nbytes, const uint32_t *__restrict__ lit_start,
                                                               const uint32_t *__restrict__ lit_len, uint32_t n_lits) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= n_lits) return;
  const size_t a = lit_start[j], l = lit_len[j];
  const bool ok = l <= static_cast<size_t>(kSpecialMaxLine) && a + l <= nbytes;
  if (!wp_in_bounds(ok, kSiteSpecial) || !ok) return;
  for (size_t k = 0; k < l; k++) copy[a + k] = 0x20u;
}

// ---- byte positions in code points: the number of valid code points in front of a byte, by the decoder's verdicts ----
// valid code points per 1 KB row of the text (decode.h's rows: the same loads and lead masks as cp_byte_kernel);
// n_rows = nbytes / 1 KB + 1, so that a position at the very end of the text has a row too
__global__ __launch_bounds__(kBlock) void special_cp_rows_kernel(const uint8_t *__restrict__ text, size_t nbytes, size_t n_rows,
                                                                 uint32_t *__restrict__ row_cnt) {
  const int lane = lane_id(), wv = wave_id();
  const size_t wave_base = static_cast<size_t>(blockIdx.x) * kDecTile + static_cast<size_t>(wv) * kDecWaveBytes;
  uint32_t w[kDecRows][5];
  dec_load_rows(text, nbytes, wave_base, lane, w);
#pragma unroll
  for (int r = 0; r < kDecRows; r++) {
    const size_t off = wave_base + static_cast<size_t>(r) * kDecRowBytes + static_cast<size_t>(lane) * kDecChunk;
    const uint32_t inside = dec_inside16(off, nbytes);
    uint32_t m = 0;
    if (((w[r][0] | w[r][1] | w[r][2] | w[r][3]) & kHi) == 0u) {
      m = inside;
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const Utf8Starts u = utf8_starts(w[r][k], w[r][k + 1]);
        m |= byte_mask4(u.v1 | u.v2 | u.v3 | u.v4) << (4 * k);
      }
      m &= inside;
    }
    const uint32_t cnt = wave_reduce_sum(__popc(m));
    const size_t row = (wave_base >> 10) + static_cast<size_t>(r);
    if (lane == 0 && row < n_rows) row_cnt[row] = cnt;
  }
}

// the word at byte pos (a multiple of 4) as the decoder sees it: bytes at or behind nbytes read as zero
__device__ __forceinline__ uint32_t special_word_at(const uint8_t *__restrict__ text, size_t nbytes, size_t pos) {
  if (pos >= nbytes) return 0u;
  uint32_t w = *reinterpret_cast<const uint32_t *>(text + pos);
  if (pos + 4 > nbytes) w &= (1u << (8 * static_cast<unsigned>(nbytes - pos))) - 1u;
  return w;
}

// valid code points in front of byte b <= nbytes (row_prefix: the exclusive scan of special_cp_rows_kernel's counts)
__device__ __forceinline__ uint32_t special_cp_before(const uint8_t *__restrict__ text, size_t nbytes, const uint32_t *__restrict__ row_prefix,
                                                      size_t b) {
  uint32_t c = row_prefix[b >> 10];
  for (size_t pos = (b >> 10) << 10; pos < b; pos += 4) {
    const uint32_t w0 = special_word_at(text, nbytes, pos);
    uint32_t m = 0xfu;
    if ((w0 & kHi) != 0u) {
      const Utf8Starts u = utf8_starts(w0, special_word_at(text, nbytes, pos + 4));
      m = byte_mask4(u.v1 | u.v2 | u.v3 | u.v4);
    }
    if (b - pos < 4) m &= (1u << static_cast<unsigned>(b - pos)) - 1u;
    c += __popc(m);
  }
  return c;
}

// What the place kernel reads of the encode of the blanked text.  starts == nullptr: the flat form (one row, [0, n_ids)).
struct SpecialRows {
  const long long *starts;      // n_rows + 1 row starts in bytes
  const long long *row_splits;  // n_rows + 1
  size_t n_rows;
};

// place: per literal its position in `unit` relative to its row, and lit_at[j] = the index among the ids of the blanked
// encode in front of which it goes (a lower bound over the span begins of its row; no span covers a blanked byte).
__global__ __launch_bounds__(kBlock) void special_place_kernel(const uint8_t *__restrict__ text, size_t nbytes, const uint32_t *__restrict__ lit_start,
                                                               uint32_t n_lits, SpecialRows rows, const uint2 *__restrict__ spans, size_t n_ids,
                                                               int unit, const uint32_t *__restrict__ row_prefix,
                                                               uint32_t *__restrict__ lit_at, uint32_t *__restrict__ lit_pos) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= n_lits) return;
  const size_t b = lit_start[j];
  size_t base = 0, lo = 0, hi = n_ids;
  if (rows.starts) {
    size_t r = 0, r_hi = rows.n_rows;  // the last row that starts at or before b
    while (r_hi - r > 1) {
      const size_t mid = r + (r_hi - r) / 2;
      if (static_cast<size_t>(rows.starts[mid]) <= b) {
        r = mid;
      } else {
        r_hi = mid;
      }
    }
    base = static_cast<size_t>(rows.starts[r]);
    lo = static_cast<size_t>(rows.row_splits[r]);
    hi = static_cast<size_t>(rows.row_splits[r + 1]);
    const bool ok = base <= b && lo <= hi && hi <= n_ids;
    if (!wp_in_bounds(ok, kSiteSpecial) || !ok) {
      base = b;
      lo = hi = min(lo, n_ids);
    }
  }
  uint32_t pos;
  if (unit == WP_OFFSETS_CODE_POINTS) {
    pos = special_cp_before(text, nbytes, row_prefix, b) - (base ? special_cp_before(text, nbytes, row_prefix, base) : 0u);
  } else {
    pos = static_cast<uint32_t>(b - base);
  }
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    if (spans[mid].x < pos) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  lit_at[j] = static_cast<uint32_t>(lo);
  lit_pos[j] = pos;
}

// number of literals whose output cell lit_at[j] + j lies at or before cell o, searched in [lo, hi]
__device__ __forceinline__ uint32_t special_lits_upto(const uint32_t *__restrict__ lit_at, uint32_t lo, uint32_t hi, size_t o) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (static_cast<size_t>(lit_at[mid]) + mid <= o) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo;
}

// merge: output cell o holds literal j where lit_at[j] + j == o, else id o - (literals in front of it) of the blanked
// encode.  One thread per cell, so ids go out as coalesced 4-byte and spans as coalesced 8-byte stores; the workgroup's
// cells lie between two literals that two of its lanes search for, which leaves every thread a short search.
// spans / out_spans == nullptr: no unit, ids only.
__global__ __launch_bounds__(kBlock) void special_merge_kernel(const int32_t *__restrict__ ids, const uint2 *__restrict__ spans, size_t n_ids,
                                                               const uint32_t *__restrict__ lit_at, const uint32_t *__restrict__ lit_pos,
                                                               const uint32_t *__restrict__ lit_len, const int32_t *__restrict__ lit_id,
                                                               uint32_t n_lits, int32_t *__restrict__ out_ids, uint2 *__restrict__ out_spans) {
  __shared__ uint32_t s_j[2];
  const size_t n_out = n_ids + n_lits;
  const size_t o0 = static_cast<size_t>(blockIdx.x) * kSpecialMergeTile;
  if (o0 >= n_out) return;
  const size_t o1 = min(n_out, o0 + static_cast<size_t>(kSpecialMergeTile));
  if (threadIdx.x == 0) s_j[0] = o0 == 0 ? 0u : special_lits_upto(lit_at, 0, n_lits, o0 - 1);
  if (threadIdx.x == kWave) s_j[1] = special_lits_upto(lit_at, 0, n_lits, o1 - 1);
  __syncthreads();
  const uint32_t j_lo = s_j[0], j_hi = s_j[1];
#pragma unroll
  for (int it = 0; it < kSpecialMergeItems; it++) {
    const size_t o = o0 + static_cast<size_t>(it) * kBlock + threadIdx.x;
    if (o >= o1) continue;
    const uint32_t upto = special_lits_upto(lit_at, j_lo, j_hi, o);  // literals at or before cell o
    if (upto > 0 && static_cast<size_t>(lit_at[upto - 1]) + (upto - 1) == o) {
      const uint32_t j = upto - 1;
      out_ids[o] = lit_id[j];
      if (out_spans) out_spans[o] = make_uint2(lit_pos[j], lit_pos[j] + lit_len[j]);
    } else {
      const size_t i = o - upto;
      const bool ok = i < n_ids;
      if (!wp_in_bounds(ok, kSiteSpecial) || !ok) {
        out_ids[o] = -1;
        if (out_spans) out_spans[o] = make_uint2(0u, 0u);
        continue;
      }
      out_ids[o] = ids[i];
      if (out_spans) out_spans[o] = spans[i];
    }
  }
}

// row_splits of the result: every boundary moves up by the literals that start in front of the row
__global__ __launch_bounds__(kBlock) void special_splits_kernel(SpecialRows rows, const uint32_t *__restrict__ lit_start, uint32_t n_lits,
                                                                long long *__restrict__ out_splits) {
  const size_t r = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (r > rows.n_rows) return;
  const unsigned long long s = static_cast<unsigned long long>(rows.starts[r]);
  uint32_t lo = 0, hi = n_lits;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (lit_start[mid] < s) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  out_splits[r] = rows.row_splits[r] + static_cast<long long>(lo);
}

}  // namespace wp
