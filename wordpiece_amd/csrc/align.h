// align.h — labelled character spans against the offsets of a batch: per-cell labels and span indices (token
// classification) and per-row start / end positions of the sample's first span (extractive QA); the contract is the
// section "span alignment" of include/wordpiece_amd.h.
//
// align_kernel has the geometry of mask_kernel (mask.h): `lanes` lanes (a power of two, 4..64) share a row, a workgroup
// holds kBlock / lanes rows, the columns of a row are taken in trips of `lanes`, and EVERY lane of a workgroup runs every
// trip.  A cell is one 8-byte coalesced load of its offsets, one 4-byte load of its type, the two split values of the
// row's sample (the same address in the whole lane group), a bisection over the ends of the sample's spans (an
// L2-resident gather; with 0 or 1 spans there is no loop) and up to two 4-byte coalesced stores.  The positions are four
// reductions over the row's lane group, carried in registers from trip to trip and stored by one lane per row.
// align_rows_kernel is the flat form over ragged rows: a tile of kBlock cells whatever the rows' lengths.
#pragma once
#include "primitives.h"

namespace wp {

struct AlignGeom {
  int max_len, side;
  int32_t outside_label, inside_add, ignore_id, no_answer;
  long long n_samples, n_spans;
};

// the counters of a call, 64 bits each, in this order behind d_scalars + kScalarAlign
enum AlignCounter { kAlignTokens = 0, kAlignCovered, kAlignBegin, kAlignAnswer, kAlignNoAnswer, kAlignCounters };

// the largest grid of a call, as kMaskMaxGrid: the counters cost one global atomic each per RESIDENT workgroup
constexpr unsigned kAlignMaxGrid = 2048;

// What the argument check found, in one 64-bit word that only grows (atomicMax; 0: nothing): the rule in the high half
// (a rule the host checks earlier is the larger number), ~detail in the low half, so that the smallest detail of the
// earliest rule stays.  detail: the entry of row_splits / span_splits, 2 * span + (0: empty, 1: begins before the span
// in front of it ends), or the row whose sample is out of range.
enum AlignRule { kAlignBadSample = 1, kAlignBadSpan = 2, kAlignBadSpanSplits = 3, kAlignBadRowSplits = 4 };
__host__ __device__ inline unsigned long long align_bad_key(int rule, unsigned long long detail) {
  return (static_cast<unsigned long long>(rule) << 32) | (0xFFFFFFFFull - detail);
}

// the first j in [j0, j1) whose span ends behind b, or j1; no loop for j1 - j0 <= 1
__device__ __forceinline__ long long align_first_end_behind(const uint2 *__restrict__ spans, long long n_spans, long long j0, long long j1,
                                                            uint32_t b, uint2 *span) {
  if (j1 <= j0) return j1;
  long long lo = j0, hi = j1 - 1;
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    uint32_t end = 0;
    if (wp_in_bounds(mid >= 0 && mid < n_spans, kSiteAlign)) end = spans[mid].y;
    if (end > b) {
      hi = mid;
    } else {
      lo = mid + 1;
    }
  }
  uint2 sp = make_uint2(0u, 0u);
  if (wp_in_bounds(lo >= 0 && lo < n_spans, kSiteAlign)) sp = spans[lo];
  *span = sp;
  return sp.y > b ? lo : j1;
}

// a wave sums its lanes' counts, LDS sums the waves, and one global atomic per counter leaves the workgroup (every lane
// of the workgroup calls this)
__device__ __forceinline__ void align_flush_counters(const unsigned long long (&sums)[kAlignCounters], unsigned long long *s_cnt,
                                                     unsigned long long *__restrict__ counters) {
#pragma unroll
  for (int k = 0; k < kAlignCounters; k++) {
    const unsigned long long v = wave_reduce_sum64(sums[k]);
    if ((threadIdx.x & (kWave - 1)) == 0 && v != 0) atomicAdd(&s_cnt[k], v);
  }
  __syncthreads();
  if (threadIdx.x < kAlignCounters && s_cnt[threadIdx.x] != 0) atomicAdd(&counters[threadIdx.x], s_cnt[threadIdx.x]);
}

// The argument rules of the device entry points, one item per thread and trip: entry i of row_splits (ragged form) and of
// span_splits, span i, row i's sample.  *bad: align_bad_key of what was found (cleared by the caller).
__global__ __launch_bounds__(kBlock) void align_check_kernel(const long long *__restrict__ row_splits, size_t n_rows, long long n_ids,
                                                             const int32_t *__restrict__ sample, const long long *__restrict__ span_splits,
                                                             size_t n_samples, const uint2 *__restrict__ spans, size_t n_spans,
                                                             unsigned long long *__restrict__ bad) {
  const size_t n_items = max(max(n_rows, n_samples) + 1, n_spans);
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n_items; i += static_cast<size_t>(gridDim.x) * kBlock) {
    if (row_splits && i <= n_rows) {
      const long long s = row_splits[i];
      if ((i == 0 && s != 0) || (i < n_rows && row_splits[i + 1] < s) || (i == n_rows && s != n_ids)) atomicMax(bad, align_bad_key(kAlignBadRowSplits, i));
    }
    if (i <= n_samples) {
      const long long s = span_splits[i];
      if ((i == 0 && s != 0) || (i < n_samples && span_splits[i + 1] < s) || (i == n_samples && s != static_cast<long long>(n_spans))) {
        atomicMax(bad, align_bad_key(kAlignBadSpanSplits, i));
      }
    }
    if (i < n_spans) {
      const uint2 sp = spans[i];
      if (sp.x >= sp.y) atomicMax(bad, align_bad_key(kAlignBadSpan, 2 * i));
      if (i + 1 < n_spans && sp.y > spans[i + 1].x) {
        // the rule holds inside a sample only: is i + 1 an entry of span_splits?  (With bad splits the search still ends
        // and stays inside the array, and the splits are what the call reports.)
        size_t lo = 0, hi = n_samples + 1;
        while (lo < hi) {
          const size_t mid = lo + (hi - lo) / 2;
          if (span_splits[mid] < static_cast<long long>(i + 1)) {
            lo = mid + 1;
          } else {
            hi = mid;
          }
        }
        if (lo > n_samples || span_splits[lo] != static_cast<long long>(i + 1)) atomicMax(bad, align_bad_key(kAlignBadSpan, 2 * (i + 1) + 1));
      }
    }
    if (i < n_rows && !row_splits) {
      const long long s = sample ? static_cast<long long>(sample[i]) : static_cast<long long>(i);
      if (s < 0 || s >= static_cast<long long>(n_samples)) atomicMax(bad, align_bad_key(kAlignBadSample, i));
    }
  }
}

// LABELS: `labels` is written; INDEX: `span_index` is; POS: `start_pos` and `end_pos` are.  offsets[n_rows * max_len] as
// (begin, end); types, lengths, sample may be nullptr (all 0; max_len; sample[r] = r).  *bad != 0: the check in front of
// this launch failed, and nothing is read or written.  n_blocks = ceil(n_rows / (kBlock / lanes)) row blocks are dealt to
// the workgroups of the grid round robin.  counters: kAlignCounters 64-bit sums.
template <bool LABELS, bool INDEX, bool POS>
__global__ __launch_bounds__(kBlock) void align_kernel(const uint2 *__restrict__ offsets, const int32_t *__restrict__ types,
                                                       const int32_t *__restrict__ lengths, const int32_t *__restrict__ sample, size_t n_rows,
                                                       size_t n_blocks, AlignGeom g, int lanes, const long long *__restrict__ span_splits,
                                                       const uint2 *__restrict__ spans, const int32_t *__restrict__ span_labels,
                                                       int32_t *__restrict__ labels, int32_t *__restrict__ span_index,
                                                       int32_t *__restrict__ start_pos, int32_t *__restrict__ end_pos,
                                                       const unsigned long long *__restrict__ bad, unsigned long long *__restrict__ counters) {
  __shared__ unsigned long long s_cnt[kAlignCounters];
  if (*bad != 0) return;  // (uniform: one word, read by every lane)
  if (threadIdx.x < kAlignCounters) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int rows_per_block = kBlock / lanes;
  const int l = threadIdx.x % lanes;  // the lane's place in its row's group
  unsigned long long n_tokens = 0, n_covered = 0, n_begin = 0, n_answer = 0, n_no_answer = 0;
  for (size_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const size_t r = blk * rows_per_block + threadIdx.x / lanes;
    const bool live = r < n_rows;
    int len = 0;
    long long j0 = 0, j1 = 0;
    if (live) {
      len = g.max_len;
      if (lengths) len = max(0, min(lengths[r], g.max_len));
      const long long s = sample ? static_cast<long long>(sample[r]) : static_cast<long long>(r);
      if (wp_in_bounds(s >= 0 && s < g.n_samples, kSiteAlign)) {
        j0 = span_splits[s];
        j1 = span_splits[s + 1];
      }
    }
    const size_t base = live ? r * static_cast<size_t>(g.max_len) : 0;
    // the answer: the first span of the sample
    uint32_t ans_b = 0, ans_e = 0;
    if (POS && j1 > j0 && wp_in_bounds(j0 >= 0 && j0 < g.n_spans, kSiteAlign)) {
      const uint2 a = spans[j0];
      ans_b = a.x;
      ans_e = a.y;
    }
    // carried from trip to trip, the lane's own share; the group's lanes are put together behind the last trip
    uint32_t lo = 0xFFFFFFFFu, hi = 0;  // min begin / max end over the token cells (hi == 0: none, a token has end > begin >= 0)
    int start_col = -1;                 // the largest token column with begin <= ans_b
    int end_col = INT32_MAX;            // the smallest token column with end >= ans_e
    // (uniform: every lane of the workgroup runs every trip; counted in 64 bits: max_len may be close to INT32_MAX)
    for (long long trip0 = 0; trip0 < g.max_len; trip0 += lanes) {
      const bool cell = live && trip0 + l < g.max_len;
      if (!cell) continue;  // (no ballot below: a lane without a cell has nothing to add to its group)
      const int col = static_cast<int>(trip0) + l;
      const uint2 o = offsets[base + col];
      const int32_t type = types ? types[base + col] : 0;
      const bool token = col < len && o.y > o.x && type == g.side;
      if (token) n_tokens++;
      if (POS && token) {
        lo = min(lo, o.x);
        hi = max(hi, o.y);
        if (o.x <= ans_b) start_col = col;  // (the columns of a lane ascend)
        if (o.y >= ans_e) end_col = min(end_col, col);
      }
      if (LABELS || INDEX) {
        int32_t label = g.ignore_id;
        long long idx = -1;
        if (token) {
          uint2 sp = make_uint2(0u, 0u);
          const long long j = align_first_end_behind(spans, g.n_spans, j0, j1, o.x, &sp);
          label = g.outside_label;
          if (j < j1 && sp.x < o.y) {
            idx = j;
            n_covered++;
            const bool begin = o.x <= sp.x;
            if (begin) n_begin++;
            if (LABELS) label = span_labels[j] + (begin ? 0 : g.inside_add);
          }
        }
        if (LABELS) labels[base + col] = label;
        if (INDEX) span_index[base + col] = static_cast<int32_t>(idx);
      }
    }
    if (POS) {
      // (every lane of the wave is here; the partners of a lane lie in its own group: lanes is a power of two <= kWave)
      for (int d = lanes / 2; d > 0; d >>= 1) {
        lo = min(lo, static_cast<uint32_t>(__shfl_xor(static_cast<int>(lo), d, kWave)));
        hi = max(hi, static_cast<uint32_t>(__shfl_xor(static_cast<int>(hi), d, kWave)));
        start_col = max(start_col, __shfl_xor(start_col, d, kWave));
        end_col = min(end_col, __shfl_xor(end_col, d, kWave));
      }
      if (live && l == 0) {
        const bool held = j1 > j0 && hi != 0 && ans_b >= lo && ans_e <= hi;
        start_pos[r] = held ? start_col : g.no_answer;
        end_pos[r] = held ? end_col : g.no_answer;
        if (held) {
          n_answer++;
        } else {
          n_no_answer++;
        }
      }
    }
  }
  const unsigned long long sums[kAlignCounters] = {n_tokens, n_covered, n_begin, n_answer, n_no_answer};
  align_flush_counters(sums, s_cnt, counters);
}

// The ragged form: offsets[n_ids] with row_splits[n_rows + 1], row i is sample i, every cell is a token.  A tile is kBlock
// consecutive cells whatever rows they lie in: two lanes find the rows of the tile's first and last cell by a bisection
// over all of row_splits, and every lane then finds its own row between those two.  n_tiles = ceil(n_ids / kBlock).
template <bool LABELS, bool INDEX>
__global__ __launch_bounds__(kBlock) void align_rows_kernel(const uint2 *__restrict__ offsets, const long long *__restrict__ row_splits,
                                                            long long n_rows, long long n_ids, size_t n_tiles, AlignGeom g,
                                                            const long long *__restrict__ span_splits, const uint2 *__restrict__ spans,
                                                            const int32_t *__restrict__ span_labels, int32_t *__restrict__ labels,
                                                            int32_t *__restrict__ span_index, const unsigned long long *__restrict__ bad,
                                                            unsigned long long *__restrict__ counters) {
  __shared__ unsigned long long s_cnt[kAlignCounters];
  __shared__ long long s_row[2];
  if (*bad != 0) return;  // (uniform)
  if (threadIdx.x < kAlignCounters) s_cnt[threadIdx.x] = 0;
  unsigned long long n_tokens = 0, n_covered = 0, n_begin = 0;
  for (size_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long first = static_cast<long long>(tile) * kBlock, last = min(first + kBlock, n_ids) - 1;
    __syncthreads();  // (s_row of the tile before is read)
    if (threadIdx.x < 2) {
      // the row of cell x: the last r in [0, n_rows) with row_splits[r] <= x (rows without cells are passed over)
      const long long x = threadIdx.x == 0 ? first : last;
      long long lo = 0, hi = n_rows - 1;
      while (lo < hi) {
        const long long mid = lo + (hi - lo + 1) / 2;
        if (row_splits[mid] <= x) {
          lo = mid;
        } else {
          hi = mid - 1;
        }
      }
      s_row[threadIdx.x] = lo;
    }
    __syncthreads();
    const long long i = first + threadIdx.x;
    if (i > last) continue;  // (the barriers above are reached by the tile count alone, which is uniform)
    long long lo = s_row[0], hi = s_row[1];
    while (lo < hi) {
      const long long mid = lo + (hi - lo + 1) / 2;
      if (row_splits[mid] <= i) {
        lo = mid;
      } else {
        hi = mid - 1;
      }
    }
    long long j0 = 0, j1 = 0;
    if (wp_in_bounds(lo >= 0 && lo < g.n_samples, kSiteAlign)) {
      j0 = span_splits[lo];
      j1 = span_splits[lo + 1];
    }
    const uint2 o = offsets[i];
    n_tokens++;
    uint2 sp = make_uint2(0u, 0u);
    const long long j = align_first_end_behind(spans, g.n_spans, j0, j1, o.x, &sp);
    int32_t label = g.outside_label;
    long long idx = -1;
    if (j < j1 && sp.x < o.y) {
      idx = j;
      n_covered++;
      const bool begin = o.x <= sp.x;
      if (begin) n_begin++;
      if (LABELS) label = span_labels[j] + (begin ? 0 : g.inside_add);
    }
    if (LABELS) labels[i] = label;
    if (INDEX) span_index[i] = static_cast<int32_t>(idx);
  }
  __syncthreads();  // (s_cnt is cleared; a workgroup without a tile has not passed a barrier yet)
  const unsigned long long sums[kAlignCounters] = {n_tokens, n_covered, n_begin, 0, 0};
  align_flush_counters(sums, s_cnt, counters);
}

}  // namespace wp
