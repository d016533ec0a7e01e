// inputs.h — model inputs on top of a rows result (wp_linear_encode_inputs): the rows of a documents call become
// samples (one row, or a pair of rows A, B), a sample becomes one output row [cls] A' [sep] (B' [sep]) pad... under a
// truncation strategy, or several overlapping windows of it (HF stride= / return_overflowing_tokens=).
//
// Two kernels, both over row_splits alone — the ids and spans are only gathered from:
//   plan   one thread per sample: how much of each side a row holds, the step between windows, the number of windows
//   pack   lanes of a wave share an output row, as in pack_rows_kernel; with windows the sample of an output row is
//          found by a search in the scanned window counts that a workgroup first narrows to the samples its rows lie
//          in (every sample has at least one row, so that is at most as many samples as the workgroup has rows)
// Between them, with windows only, device_exclusive_scan over the window counts.
#pragma once
#include "rows.h"

namespace wp {

struct InputsGeom {
  int max_len, head, nsep;  // head: 1 with a [cls]; nsep: 1 with a [sep]
  int budget;               // B = max_len - specials
  int pairs, truncation, stride;
  int32_t cls_id, sep_id, pad_id;
};

// What the packer needs of a sample: cap_a / cap_b ids of A / B at most in one output row; side 1 / 2: A / B is cut
// into windows that start `step` ids apart (0: neither, one row).
struct InputsRec {
  uint32_t cap_a, cap_b, step, side;
};
static_assert(sizeof(InputsRec) == 16, "one 16-byte record per sample");

// The contract's arithmetic for one sample (include/wordpiece_amd.h, "model inputs"): -> the number of output rows
__device__ __forceinline__ uint32_t inputs_plan_one(long long la, long long lb, const InputsGeom &g, InputsRec &rec, bool &cut) {
  const long long B = g.budget;
  if (g.truncation == WP_TRUNC_LONGEST_FIRST) {
    long long ka = la, kb = lb;
    if (la + lb > B) {
      if (la <= lb) {
        ka = min(la, max(B - lb, B / 2));
        kb = min(lb, B - ka);
      } else {
        kb = min(lb, max(B - la, B / 2));
        ka = min(la, B - kb);
      }
    }
    rec = InputsRec{static_cast<uint32_t>(ka), static_cast<uint32_t>(kb), 0u, 0u};
    cut = ka < la || kb < lb;
    return 1u;
  }
  const long long st = g.stride > 0 ? g.stride : 0;
  const bool win_a = g.pairs == 0 || g.truncation == WP_TRUNC_ONLY_FIRST;
  const long long l = win_a ? la : lb, lF = g.pairs == 0 ? 0 : (win_a ? lb : la);
  const long long kF = min(lF, B - st - 1);  // (B >= st + 1 is checked on the host)
  const long long W = B - kF, step = W - st;
  const bool all = g.stride >= 0;
  const long long n_win = (l <= W || !all) ? 1 : 1 + (l - W + step - 1) / step;
  rec = InputsRec{static_cast<uint32_t>(win_a ? W : kF), static_cast<uint32_t>(win_a ? kF : W), static_cast<uint32_t>(step),
                  win_a ? 1u : 2u};
  cut = kF < lF || (!all && l > W);
  return static_cast<uint32_t>(n_win);
}

// n_win[s], rec[s] per sample; *n_cut += samples that lost ids for good, *n_windowed += samples with more than one
// window (one global atomic each per workgroup at most)
__global__ __launch_bounds__(kBlock) void inputs_plan_kernel(const long long *__restrict__ row_splits, size_t n_samples, InputsGeom g,
                                                             uint32_t *__restrict__ n_win, InputsRec *__restrict__ rec,
                                                             uint32_t *__restrict__ n_cut, uint32_t *__restrict__ n_windowed) {
  __shared__ uint32_t s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s < n_samples) {
    const size_t i = g.pairs ? 2 * s : s;
    const long long a = row_splits[i], m = row_splits[i + 1], e = g.pairs ? row_splits[i + 2] : m;
    InputsRec q;
    bool cut;
    const uint32_t w = inputs_plan_one(m - a, e - m, g, q, cut);
    n_win[s] = w;
    rec[s] = q;
    if (cut) atomicAdd(&s_cnt[0], 1u);
    if (w > 1) atomicAdd(&s_cnt[1], 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt[0] != 0) atomicAdd(n_cut, s_cnt[0]);
  if (threadIdx.x == kWave && s_cnt[1] != 0) atomicAdd(n_windowed, s_cnt[1]);
}

// last s in [lo, hi) with first[s] <= r (first[lo] <= r is given)
__device__ __forceinline__ size_t sample_of_row(const uint32_t *__restrict__ first, size_t lo, size_t hi, size_t r) {
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (first[mid] <= r) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  return lo;
}

// Output row r = window r - first[s] of its sample s (first == nullptr: one row per sample, s = r).  `lanes` as in
// pack_rows_kernel.  offs / out_offs: the spans of the ids and their place in the batch ([n_out, max_len] pairs), or
// out_offs == nullptr.  Nothing behind row n_out is written.
__global__ __launch_bounds__(kBlock) void inputs_pack_kernel(const int32_t *__restrict__ ids, const uint2 *__restrict__ offs, size_t n_ids,
                                                             const long long *__restrict__ row_splits, const InputsRec *__restrict__ rec,
                                                             const uint32_t *__restrict__ first, size_t n_samples, size_t n_out,
                                                             InputsGeom g, int lanes, int32_t *__restrict__ input_ids,
                                                             int32_t *__restrict__ type_ids, uint2 *__restrict__ out_offs,
                                                             int32_t *__restrict__ lengths, int32_t *__restrict__ sample) {
  __shared__ unsigned long long s_rng[2];
  const int rows_per_block = kBlock / lanes;
  const size_t r0 = static_cast<size_t>(blockIdx.x) * rows_per_block;
  if (r0 >= n_out) return;
  if (first) {
    const size_t r1 = min(n_out, r0 + static_cast<size_t>(rows_per_block)) - 1;
    if (threadIdx.x == 0) s_rng[0] = sample_of_row(first, 0, n_samples, r0);
    if (threadIdx.x == kWave) s_rng[1] = sample_of_row(first, 0, n_samples, r1);
    __syncthreads();
  }
  const size_t r = r0 + threadIdx.x / lanes;
  const int col0 = threadIdx.x % lanes;
  if (r >= n_out) return;
  size_t s = r;
  long long j = 0;  // the window
  if (first) {
    s = sample_of_row(first, s_rng[0], s_rng[1] + 1, r);
    j = static_cast<long long>(r - first[s]);
  }
  const size_t i = g.pairs ? 2 * s : s;
  const long long a = row_splits[i], m = row_splits[i + 1], e = g.pairs ? row_splits[i + 2] : m;
  const InputsRec q = rec[s];
  const long long a_off = q.side == 1 ? j * q.step : 0, b_off = q.side == 2 ? j * q.step : 0;
  const int a_cnt = static_cast<int>(max(0ll, min(m - a - a_off, static_cast<long long>(q.cap_a))));
  const int b_cnt = static_cast<int>(max(0ll, min(e - m - b_off, static_cast<long long>(q.cap_b))));
  const long long a_src = a + a_off, b_src = m + b_off;
  const int a_end = g.head + a_cnt;         // first [sep]
  const int b_beg = a_end + g.nsep;         // B' (pairs)
  const int b_end = b_beg + b_cnt;          // second [sep] (pairs)
  const int len = g.pairs ? b_end + g.nsep : b_beg;
  const size_t base = r * static_cast<size_t>(g.max_len);
  for (int col = col0; col < g.max_len; col += lanes) {
    int32_t x = g.pad_id;
    long long src = -1;
    if (col < g.head) {
      x = g.cls_id;
    } else if (col < a_end) {
      src = a_src + (col - g.head);
    } else if (col < b_beg) {
      x = g.sep_id;
    } else if (g.pairs && col < b_end) {
      src = b_src + (col - b_beg);
    } else if (g.pairs && col < len) {
      x = g.sep_id;
    }
    uint2 sp = make_uint2(0u, 0u);
    if (src >= 0) {
      const bool ok = static_cast<unsigned long long>(src) < n_ids;
      if (wp_in_bounds(ok, kSiteInputs) && ok) {
        x = ids[src];
        if (out_offs) sp = offs[src];
      }
    }
    input_ids[base + col] = x;
    type_ids[base + col] = (g.pairs && col >= b_beg && col < len) ? 1 : 0;
    if (out_offs) out_offs[base + col] = sp;
  }
  if (col0 == 0) {
    lengths[r] = len;
    sample[r] = static_cast<int32_t>(s);
  }
}

}  // namespace wp
