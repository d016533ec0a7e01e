// rows.h — the documents layer on top of offsets mode (wp_linear_encode_rows / wp_linear_encode_padded): the rows of a
// joined text (documents back to back, each followed by one '\n'), the split of the id list into rows, offsets relative
// to the id's own document, and padded [n_rows, max_len] batches.
//
// Row membership is a function of the spans offsets mode leaves in HBM (offsets.h): an id belongs to the last document
// that starts at or before its span.  Document starts are bytes, the walk's spans are code points, so a start is first
// mapped to its code point by a search in byte_of[] (built for both units in a documents call), then to an id by a
// lower bound over the span begins.  Two searches per row, nothing per id; the rebase is one pass of its own over the
// 8-byte spans (after span_bytes_kernel in the byte unit), which finds the row of an id by a search that a workgroup
// first narrows to the rows its 2048 ids can lie in.
#pragma once
#include "offsets.h"

namespace wp {

constexpr int kLineIters = 4;
constexpr int kLineTile = kBlock * kDecChunk * kLineIters;  // 16 KB of text per workgroup
constexpr int kRebaseItems = 8;
constexpr int kRebaseTile = kBlock * kRebaseItems;  // ids per workgroup of the rebase

// Which of the 16 bytes at `off` end a line (bit j: byte off + j): a '\n', or the last byte of the text whatever it is
// (a text that does not end in '\n' has a last line that runs to the end; one that does has no extra empty row).
// text: 4-byte aligned and readable up to the next multiple of 16 behind nbytes; off: a multiple of 16.
__device__ __forceinline__ uint32_t line_ends16(const uint8_t *__restrict__ text, size_t nbytes, size_t off) {
  if (off >= nbytes) return 0u;
  const dec_u32x4 v = *reinterpret_cast<const dec_u32x4 *>(text + off);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t x = w[k] ^ 0x0a0a0a0au;  // a zero byte where the text has '\n'
    const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & kHi;
    m |= byte_mask4(z) << (4 * k);
  }
  m &= dec_inside16(off, nbytes);  // (the tail behind nbytes is padding)
  if (nbytes - off <= static_cast<size_t>(kDecChunk)) m |= 1u << static_cast<unsigned>(nbytes - 1 - off);
  return m;
}

// lines mode, pass 1: line ends per tile
__global__ __launch_bounds__(kBlock) void line_count_kernel(const uint8_t *__restrict__ text, size_t nbytes,
                                                            uint32_t *__restrict__ tile_cnt) {
  __shared__ uint32_t sm[8];
  const size_t tile_base = static_cast<size_t>(blockIdx.x) * kLineTile;
  uint32_t cnt = 0;
#pragma unroll
  for (int j = 0; j < kLineIters; j++) {
    const size_t off = tile_base + (static_cast<size_t>(j) * kBlock + threadIdx.x) * kDecChunk;
    cnt += __popc(line_ends16(text, nbytes, off));
  }
  uint32_t total;
  (void)block_excl_sum(cnt, sm, total);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// lines mode, pass 2: starts[0] = 0, starts[1 + k] = one past the k-th line end (tile_prefix: the exclusive scan of pass 1)
__global__ __launch_bounds__(kBlock) void line_write_kernel(const uint8_t *__restrict__ text, size_t nbytes,
                                                            const uint32_t *__restrict__ tile_prefix, size_t n_rows,
                                                            long long *__restrict__ starts) {
  __shared__ uint32_t sm[8];
  const size_t tile_base = static_cast<size_t>(blockIdx.x) * kLineTile;
  if (blockIdx.x == 0 && threadIdx.x == 0) starts[0] = 0;
  size_t carry = tile_prefix[blockIdx.x];
#pragma unroll
  for (int j = 0; j < kLineIters; j++) {
    const size_t off = tile_base + (static_cast<size_t>(j) * kBlock + threadIdx.x) * kDecChunk;
    uint32_t m = line_ends16(text, nbytes, off);
    uint32_t total;
    size_t o = carry + block_excl_sum(__popc(m), sm, total) + 1;
    while (m) {
      const int b = __ffs(static_cast<int>(m)) - 1;
      m &= m - 1u;
      if (wp_in_bounds(o <= n_rows, kSiteSpan) && o <= n_rows) starts[o] = static_cast<long long>(off + static_cast<size_t>(b) + 1);
      o++;
    }
    carry += total;
  }
}

// explicit rows: one thread per boundary — doc_off[0] == 0, increasing, in range, doc_off[n_docs] == nbytes, and the byte
// in front of every boundary behind the first is the separator.  *bad counts the boundaries that fail.
__global__ __launch_bounds__(kBlock) void rows_check_kernel(const uint8_t *__restrict__ text, size_t nbytes,
                                                            const long long *__restrict__ doc_off, size_t n_docs,
                                                            uint32_t *__restrict__ bad) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i > n_docs) return;
  const long long b = doc_off[i];
  bool ok;
  if (i == 0) {
    ok = b == 0;
  } else {
    ok = b > doc_off[i - 1] && b >= 1 && static_cast<unsigned long long>(b) <= nbytes;
    if (ok) ok = text[b - 1] == 0x0au;
  }
  if (i == n_docs) ok = ok && static_cast<unsigned long long>(b) == nbytes;
  if (!ok) atomicAdd(bad, 1u);
}

// first code point that starts at or behind byte b: the first p in [0, n_text) with byte_of[p] >= b (n_text: none).
// byte_of[p] >= p (a code point has at least one byte), so the answer is at most b, and in ASCII text it is b itself:
// the search gallops down from min(b, n_text) — two loads where the text in front of b is ASCII — then bisects.
__device__ __forceinline__ size_t cp_at_byte(const uint32_t *__restrict__ byte_of, size_t n_text, unsigned long long b) {
  size_t hi = static_cast<size_t>(min(b, static_cast<unsigned long long>(n_text)));  // byte_of[hi] >= b, or hi == n_text
  size_t lo = 0;  // everything below lo starts in front of b
  for (size_t step = 1; hi > 0; step *= 2) {
    const size_t q = hi > step ? hi - step : 0;
    if (byte_of[q] < b) {
      lo = q + 1;
      break;
    }
    hi = q;
  }
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    if (byte_of[mid] < b) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo;
}

// row_splits[i] = number of ids whose span begins before document i (i = n_rows: all of them); row_base[i] = the start
// of document i in `unit` (bytes: starts[i]; code points: its first code point).  spans: [begin, end) per id in code
// points, increasing (the walk's result, before span_bytes_kernel).
__global__ __launch_bounds__(kBlock) void row_splits_kernel(const long long *__restrict__ starts, size_t n_rows,
                                                            const uint32_t *__restrict__ byte_of, size_t n_text,
                                                            const uint2 *__restrict__ spans, size_t n_ids, int unit,
                                                            long long *__restrict__ row_splits, uint32_t *__restrict__ row_base) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i > n_rows) return;
  const unsigned long long b = static_cast<unsigned long long>(starts[i]);
  const size_t p = cp_at_byte(byte_of, n_text, b);
  size_t lo = 0, hi = n_ids;
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    if (spans[mid].x < p) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  row_splits[i] = static_cast<long long>(lo);
  if (row_base) row_base[i] = unit == WP_OFFSETS_BYTES ? static_cast<uint32_t>(b) : static_cast<uint32_t>(p);
}

// last r in [lo, hi) with row_splits[r] <= k (row_splits[lo] <= k is given)
__device__ __forceinline__ size_t row_of_id(const long long *__restrict__ row_splits, size_t lo, size_t hi, size_t k) {
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (static_cast<size_t>(row_splits[mid]) <= k) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  return lo;
}

// offs[k] -= row_base[row of id k] (in place).  The workgroup's ids lie in the rows [row of its first id, row of its
// last id]: two full searches per workgroup, a short one per id.
__global__ __launch_bounds__(kBlock) void rebase_kernel(uint2 *__restrict__ offs, size_t n_ids, const long long *__restrict__ row_splits,
                                                        size_t n_rows, const uint32_t *__restrict__ row_base) {
  __shared__ unsigned long long s_row[2];
  const size_t k0 = static_cast<size_t>(blockIdx.x) * kRebaseTile;
  if (k0 >= n_ids) return;
  const size_t k1 = min(n_ids, k0 + static_cast<size_t>(kRebaseTile));
  uint2 sp[kRebaseItems];  // (the workgroup's spans are on their way while two of its lanes search)
#pragma unroll
  for (int j = 0; j < kRebaseItems; j++) {
    const size_t k = k0 + static_cast<size_t>(j) * kBlock + threadIdx.x;
    sp[j] = k < k1 ? offs[k] : make_uint2(0u, 0u);
  }
  if (threadIdx.x == 0) s_row[0] = row_of_id(row_splits, 0, n_rows, k0);
  if (threadIdx.x == kWave) s_row[1] = row_of_id(row_splits, 0, n_rows, k1 - 1);
  __syncthreads();
  const size_t r_lo = s_row[0], r_hi = s_row[1];
#pragma unroll
  for (int j = 0; j < kRebaseItems; j++) {
    const size_t k = k0 + static_cast<size_t>(j) * kBlock + threadIdx.x;
    if (k >= k1) continue;
    const size_t r = row_of_id(row_splits, r_lo, r_hi + 1, k);
    const uint32_t base = row_base[r];
    const uint2 s = sp[j];
    const bool ok = s.x >= base;
    if (!wp_in_bounds(ok, kSiteSpan) || !ok) {
      offs[k] = make_uint2(0u, 0u);
      continue;
    }
    offs[k] = make_uint2(s.x - base, s.y - base);
  }
}

// Ragged rows given in device memory (detokenize, pack): splits[0] == 0, no descent.  bad: violations; last: splits[n_rows].
__global__ __launch_bounds__(kBlock) void check_splits_kernel(const long long *__restrict__ splits, size_t n_rows,
                                                              uint32_t *__restrict__ bad, long long *__restrict__ last) {
  for (size_t r = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; r <= n_rows; r += static_cast<size_t>(gridDim.x) * kBlock) {
    const long long s = splits[r];
    if (s < 0 || (r == 0 && s != 0) || (r < n_rows && splits[r + 1] < s)) atomicAdd(bad, 1u);
    if (r == n_rows) *last = s;
  }
}

// lanes of a wave that share a row of max_len cells (pack_rows_kernel, inputs_pack_kernel, mask_kernel)
static int lanes_for(int max_len) {
  int lanes = 4;
  while (lanes < kWave && lanes < max_len) lanes *= 2;
  return lanes;
}

// Padded batch: row r of input_ids[n_rows, max_len] = [cls] + T[:keep] + [sep] + pad..., T = ids[row_splits[r] :
// row_splits[r + 1]], keep = min(len(T), max_len - specials); lengths[r] = keep + specials.  cls_id / sep_id < 0: none.
// `lanes` (a power of two, 4..64, >= max_len where that is <= 64) lanes share a row, so a wave holds 64 / lanes short
// rows and its stores run along consecutive rows of the output; *truncated += rows that lost ids (one atomic per
// workgroup at most).
__global__ __launch_bounds__(kBlock) void pack_rows_kernel(const int32_t *__restrict__ ids, const long long *__restrict__ row_splits,
                                                           size_t n_rows, int max_len, int32_t cls_id, int32_t sep_id, int32_t pad_id,
                                                           int lanes, int32_t *__restrict__ input_ids, int32_t *__restrict__ lengths,
                                                           uint32_t *__restrict__ truncated) {
  __shared__ uint32_t s_trunc;
  if (threadIdx.x == 0) s_trunc = 0;
  __syncthreads();
  const int rows_per_block = kBlock / lanes;
  const size_t r = static_cast<size_t>(blockIdx.x) * rows_per_block + threadIdx.x / lanes;
  const int col0 = threadIdx.x % lanes;
  if (r < n_rows) {
    const long long a = row_splits[r], len = row_splits[r + 1] - a;
    const int head = cls_id >= 0 ? 1 : 0, specials = head + (sep_id >= 0 ? 1 : 0);
    const int keep = static_cast<int>(min(len, static_cast<long long>(max_len - specials)));
    int32_t *out = input_ids + r * static_cast<size_t>(max_len);
    for (int col = col0; col < max_len; col += lanes) {
      int32_t x = pad_id;
      if (col < head) {
        x = cls_id;
      } else if (col < head + keep) {
        x = ids[a + (col - head)];
      } else if (col == head + keep && sep_id >= 0) {
        x = sep_id;
      }
      out[col] = x;
    }
    if (col0 == 0) {
      lengths[r] = keep + specials;
      if (len > keep) atomicAdd(&s_trunc, 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_trunc != 0) atomicAdd(truncated, s_trunc);
}

}  // namespace wp
