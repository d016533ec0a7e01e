// neardup.h — the kernels of the near-duplicate row clustering (include/wordpiece_amd.h, section "near-duplicate rows";
// host path: neardup_path.h).  The input is dedup's ragged batch.  A row of L elements has max(L - k + 1, 1) shingle
// positions (none where L == 0), and all work on the data is flat over the positions of the batch: a tile of kNearTile
// positions finds its rows by bisection in the scanned position counts, so one row of 10^8 elements costs what 10^6
// rows of 100 do and no lane, wave or workgroup walks a row.  A workgroup hashes every shingle of its tile once into
// LDS; then each of its four waves walks one segment of kNearSeg positions with lane l holding the permutations l,
// l + 64, ... in registers: every lane of a wave is at the same position, so a row boundary is the same branch in all
// of them.  A row that lies inside one segment leaves with a plain coalesced store, a row that spans segments with
// atomicMin on signatures that start at 0xffffffff.  Band keys are one lane per (row, band); the buckets are the runs
// of one stable sort over all of them (the head kernels of group.h); the members of a run that are not of the
// head's row are compacted into the candidate list, every candidate is compared with its head by a group of 16 lanes,
// and the surviving (member, head) pairs are the edges.  Components: rounds of
// "hook the larger label to the smaller" by atomicMin over the edge list, each followed by pointer jumping; no kernel
// waits for another workgroup.  The label array then goes through the table and compact-form kernels of group.h.
#pragma once
#include "common.h"
#include "group.h"  // mix64, word_at, last_le, run_of, ragged_row; the round, table and compact-form kernels run beside these

namespace wp {

constexpr int kNearTile = 1024;                              // T: shingle positions per workgroup
constexpr int kNearSeg = kNearTile / (kBlock / kWave);       // positions a wave walks
constexpr int kNearMaxShingle = 64;                          // elements of a shingle, at most
constexpr int kNearMaxPerm = 256;                            // permutations, at most
constexpr int kNearMaxSlots = kNearMaxPerm / kWave;          // permutations a lane holds, at most
constexpr int kNearEdgeLanes = 16;                           // lanes that compare one member with its head
constexpr uint32_t kNearNoRow = 0xffffffffu;
constexpr uint64_t kNearG = kGolden;                          // (the contract's name for it)
static_assert(kNearSeg % kWave == 0 && kNearTile == kNearSeg * (kBlock / kWave), "a wave walks whole chunks of 64 positions");

// the counters of a call, 64 bits each, in d_scalars from kScalarNear on
enum NearCounter { kNearEmpty = 0, kNearBuckets = 1, kNearCounters = 4 };

// Row i through ragged_row (offsets checked, byte_off, *n_elems), then its shingle positions, whether it has any, and
// its first label (itself).  Entry n_rows closes n_pos and has (0) for their scans.  Counted: the empty rows.
__global__ __launch_bounds__(kBlock) void near_rows_kernel(const long long *__restrict__ row_off, size_t n_rows, uint32_t elem_bytes, uint32_t k,
                                                           uint32_t *__restrict__ byte_off, uint32_t *__restrict__ n_pos,
                                                           uint32_t *__restrict__ has, int32_t *__restrict__ label, uint32_t *__restrict__ bad,
                                                           unsigned long long *__restrict__ n_elems, unsigned long long *__restrict__ counters) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  bool empty = false;
  if (i <= n_rows) {
    const RaggedRow r = ragged_row(row_off, n_rows, elem_bytes, i, byte_off, bad, n_elems);
    if (!r.row) {
      n_pos[i] = 0;
      has[i] = 0;
    } else {
      const unsigned long long np = r.len == 0 ? 0ull : (r.len >= k ? r.len - k + 1 : 1ull);
      n_pos[i] = static_cast<uint32_t>(np > 0xffffffffull ? 0xffffffffull : np);
      has[i] = r.len != 0 ? 1u : 0u;
      label[i] = static_cast<int32_t>(i);
      empty = r.len == 0;
    }
  }
  const uint32_t e = wave_reduce_sum(empty ? 1u : 0u);
  if (lane_id() == 0 && e != 0) atomicAdd(counters + kNearEmpty, static_cast<unsigned long long>(e));
}

// The 32-bit value of the shingle at the bytes [s, s + B) of the data (1 <= B <= 256): the contract's shingle hash.
// The loads are word_at's: aligned words that begin below s + B, masked behind it.
__device__ __forceinline__ uint32_t near_shingle_x32(const uint32_t *__restrict__ d32, size_t s, uint32_t B, uint64_t seed) {
  const size_t e = s + B;
  uint64_t h = mix64(mix64(seed ^ kNearG) ^ (static_cast<uint64_t>(B) | (1ull << 41)));
  const uint32_t full = min(B >> 3, static_cast<uint32_t>(kNearMaxShingle * 4 / 8));
  for (uint32_t q = 0; q < full; q++) {
    const uint64_t x = static_cast<uint64_t>(word_at(d32, s, e, 2 * q)) | (static_cast<uint64_t>(word_at(d32, s, e, 2 * q + 1)) << 32);
    h = mix64(h ^ x) + kNearG;
  }
  const uint32_t rest = B & 7u;
  uint64_t x = 0;
  if (rest != 0) x = word_at(d32, s, e, 2 * full);
  if (rest > 4) x |= static_cast<uint64_t>(word_at(d32, s, e, 2 * full + 1)) << 32;
  h = mix64(h ^ x);
  return static_cast<uint32_t>(h ^ (h >> 32));
}

// Tile blockIdx.x of the shingle positions [0, n_positions) (pos_off: the exclusive scan of n_pos, n_rows + 1 entries).
// Phase 1, one lane per position: its row by bisection, its shingle's value and its row into LDS.
// Phase 2, wave w over the positions [w * kNearSeg, (w + 1) * kNearSeg) of the tile: lane l keeps the running minimum
// of the permutations l + 64 q, q < SLOTS, and the wave stores them where the row changes and at the end of the
// segment — plainly where the row's positions lie inside the segment, by atomicMin where they do not (sig starts at
// 0xffffffff everywhere).  The position and its row come out of a lane of a 64-position chunk by v_readlane: they are
// wave-uniform, and so is every branch on them.
template <int SLOTS>
__global__ __launch_bounds__(kBlock) void near_sig_kernel(const uint32_t *__restrict__ d32, size_t n_bytes, const uint32_t *__restrict__ byte_off,
                                                          const uint32_t *__restrict__ pos_off, size_t n_rows, size_t n_positions,
                                                          uint32_t elem_bytes, uint32_t k, uint32_t n_perm, uint64_t seed,
                                                          uint32_t *__restrict__ sig) {
  __shared__ uint32_t s_x[kNearTile];
  __shared__ uint32_t s_row[kNearTile];
  const size_t p0 = static_cast<size_t>(blockIdx.x) * kNearTile;
  for (int t = threadIdx.x; t < kNearTile; t += kBlock) {
    const size_t p = p0 + t;
    uint32_t x = 0, row = kNearNoRow;
    if (p < n_positions) {
      const size_t lo = last_le(pos_off, size_t(0), n_rows, p);  // the row that holds p (rows without positions are passed)
      const size_t r0 = byte_off[lo], r1 = byte_off[lo + 1];
      const size_t at = (p - pos_off[lo]) * elem_bytes;
      const bool inside = r0 < r1 && r1 <= n_bytes && pos_off[lo] <= p && at < r1 - r0;
      if (wp_checked(inside, kSiteNearDup)) {
        const uint32_t B = static_cast<uint32_t>(min(r1 - r0, static_cast<size_t>(k) * elem_bytes));
        const bool fits = r0 + at + B <= r1;
        if (wp_checked(fits, kSiteNearDup)) {
          x = near_shingle_x32(d32, r0 + at, B, seed);
          row = static_cast<uint32_t>(lo);
        }
      }
    }
    s_x[t] = x;
    s_row[t] = row;
  }
  __syncthreads();
  const int lane = lane_id();
  const int seg0 = wave_id() * kNearSeg;
  const size_t seg_begin = p0 + seg0;
  if (seg_begin >= n_positions) return;
  const int cnt = static_cast<int>(min(static_cast<size_t>(kNearSeg), n_positions - seg_begin));
  const size_t seg_end = seg_begin + cnt;
  uint64_t a[SLOTS], b[SLOTS];
  uint32_t m[SLOTS];
#pragma unroll
  for (int q = 0; q < SLOTS; q++) {
    const uint64_t j = static_cast<uint64_t>(lane + kWave * q);
    a[q] = mix64(seed + (2 * j + 1) * kNearG);
    b[q] = mix64(seed + (2 * j + 2) * kNearG);
    m[q] = 0xffffffffu;
  }
  // the minima of row `row` so far leave the wave, and start again
  auto flush = [&](uint32_t row) {
    if (row != kNearNoRow && row < n_rows) {
      const bool whole = pos_off[row] >= seg_begin && pos_off[row + 1] <= seg_end;
#pragma unroll
      for (int q = 0; q < SLOTS; q++) {
        const uint32_t j = static_cast<uint32_t>(lane + kWave * q);
        if (j < n_perm) {
          uint32_t *dst = sig + static_cast<size_t>(row) * n_perm + j;
          if (whole) *dst = m[q]; else atomicMin(dst, m[q]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < SLOTS; q++) m[q] = 0xffffffffu;
  };
  uint32_t cur = kNearNoRow;
  for (int c0 = 0; c0 < cnt; c0 += kWave) {
    const uint32_t xv = s_x[seg0 + c0 + lane], rv = s_row[seg0 + c0 + lane];
    const int lim = min(kWave, cnt - c0);
    for (int t = 0; t < lim; t++) {
      const uint32_t row = static_cast<uint32_t>(__builtin_amdgcn_readlane(rv, t));
      const uint64_t x = static_cast<uint32_t>(__builtin_amdgcn_readlane(xv, t));  // (the builtin returns int: no sign extension)
      if (row != cur) {
        flush(cur);
        cur = row;
      }
#pragma unroll
      for (int q = 0; q < SLOTS; q++) m[q] = min(m[q], static_cast<uint32_t>((a[q] * x + b[q]) >> 32));
    }
  }
  flush(cur);
}

// key[q] of item q = (slot of a row with shingles) * bands + band: the contract's band key over the r signature
// entries of that band.  rows: the rows with shingles, ascending, so the items ascend by row and then by band.
__global__ __launch_bounds__(kBlock) void near_band_keys_kernel(const uint32_t *__restrict__ sig, const uint32_t *__restrict__ rows, size_t n_items,
                                                                size_t n_rows, uint32_t n_perm, uint32_t bands, uint64_t seed,
                                                                uint64_t *__restrict__ key) {
  const size_t q = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (q >= n_items) return;
  const uint32_t row = rows[q / bands], band = static_cast<uint32_t>(q % bands);
  const uint32_t r = min(n_perm / bands, static_cast<uint32_t>(kNearMaxPerm));
  uint64_t h = mix64(mix64(seed ^ kNearG) ^ (static_cast<uint64_t>(band) + (1ull << 42)));
  if (wp_checked(row < n_rows, kSiteNearDup)) {
    const uint32_t *s = sig + static_cast<size_t>(row) * n_perm + static_cast<size_t>(band) * r;
    for (uint32_t t = 0; t < r; t++) h = mix64(h ^ s[t]) + kNearG;
  }
  key[q] = h;
}

// Sorted position s: the member's row and the row of its run's head (the sort is stable and the items ascend, so the
// head is the run's smallest row).  A member of another row than the head is a candidate: cand[s], and its two rows.
// Counted: the runs of more than one member.
__global__ __launch_bounds__(kBlock) void near_match_kernel(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ val,
                                                            const uint32_t *__restrict__ head, const uint32_t *__restrict__ run,
                                                            const uint32_t *__restrict__ head_pos, size_t n_items, size_t n_rows, uint32_t bands,
                                                            uint32_t *__restrict__ cand, uint32_t *__restrict__ member_row,
                                                            uint32_t *__restrict__ head_row, unsigned long long *__restrict__ counters) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  bool is_cand = false, bucket = false;
  uint32_t mrow = 0, hrow = 0;
  if (s < n_items) {
    const uint32_t r = run_of(head, run, s);
    if (wp_checked(r < n_items && val[s] < n_items, kSiteNearDup)) {
      const uint32_t hs = head_pos[r];
      if (wp_checked(hs <= s && val[hs] < n_items, kSiteNearDup)) {
        mrow = rows[val[s] / bands];
        hrow = rows[val[hs] / bands];
        if (wp_checked(mrow < n_rows && hrow <= mrow, kSiteNearDup)) {
          is_cand = hs != s && mrow != hrow;
          bucket = hs == s && head_pos[r + 1] - hs > 1u;
        }
      }
    }
    cand[s] = is_cand ? 1u : 0u;
    member_row[s] = mrow;
    head_row[s] = hrow;
  }
  const uint32_t nb = wave_reduce_sum(bucket ? 1u : 0u);
  if (lane_id() == 0 && nb != 0) atomicAdd(counters + kNearBuckets, static_cast<unsigned long long>(nb));
}

// Candidate c, by a group of kNearEdgeLanes lanes and coalesced reads: pass[c] = 1 where at least min_agree of the n_perm
// signature entries of the member and of the head agree.
__global__ __launch_bounds__(kBlock) void near_agree_kernel(const uint32_t *__restrict__ sig, const uint32_t *__restrict__ member_row,
                                                            const uint32_t *__restrict__ head_row, size_t n_cand, size_t n_rows, uint32_t n_perm,
                                                            uint32_t min_agree, uint32_t *__restrict__ pass) {
  const size_t c = (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x) / kNearEdgeLanes;
  const uint32_t sub = threadIdx.x % kNearEdgeLanes;
  uint32_t agree = 0;
  if (c < n_cand) {
    const uint32_t mrow = member_row[c], hrow = head_row[c];
    if (wp_checked(mrow < n_rows && hrow < n_rows, kSiteNearDup)) {
      const uint32_t *ms = sig + static_cast<size_t>(mrow) * n_perm, *hs = sig + static_cast<size_t>(hrow) * n_perm;
      for (uint32_t j = sub; j < n_perm && j < static_cast<uint32_t>(kNearMaxPerm); j += kNearEdgeLanes) agree += ms[j] == hs[j] ? 1u : 0u;
    }
  }
#pragma unroll
  for (int d = kNearEdgeLanes / 2; d > 0; d >>= 1) agree += __shfl_xor(agree, d, kWave);
  if (sub == 0 && c < n_cand) pass[c] = agree >= min_agree ? 1u : 0u;
}

// One round over the edge list: where the labels of an edge's rows differ, the larger label's row takes the smaller
// label by atomicMin, whichever end it came from; *changed = 1 where a label fell.  Labels only fall and are always rows
// of the same component, so a value read late costs a round, never a result.
__global__ __launch_bounds__(kBlock) void near_hook_kernel(const uint32_t *__restrict__ eu, const uint32_t *__restrict__ ev, size_t n_edges,
                                                           size_t n_rows, int32_t *label, uint32_t *__restrict__ changed) {
  const size_t e = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= n_edges) return;
  const uint32_t u = eu[e], v = ev[e];
  if (!wp_checked(u < n_rows && v < n_rows, kSiteNearDup)) return;
  const int32_t lu = label[u], lv = label[v];
  if (lu == lv) return;
  const int32_t lo = min(lu, lv), hi = max(lu, lv);
  if (!wp_checked(lo >= 0 && static_cast<size_t>(hi) < n_rows, kSiteNearDup)) return;
  if (atomicMin(label + hi, lo) > lo) *changed = 1u;
}

// Pointer jumping: label[i] = the end of the chain label[label[...]] from i.  A chain descends strictly, so it ends
// within n_rows steps, and the loop says so.
__global__ __launch_bounds__(kBlock) void near_jump_kernel(int32_t *label, size_t n_rows) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n_rows) return;
  int32_t l = label[i];
  for (size_t step = 0; step < n_rows; step++) {
    const bool ok = l >= 0 && static_cast<size_t>(l) < n_rows;
    if (!wp_checked(ok, kSiteNearDup)) return;
    const int32_t up = label[l];
    if (up >= l) break;
    l = up;
  }
  label[i] = l;
}

// row_count[cluster[i]] += 1: the sizes of the components, by integer atomics (row_count starts at 0)
__global__ __launch_bounds__(kBlock) void near_sizes_kernel(const int32_t *__restrict__ cluster, size_t n_rows, uint32_t *__restrict__ row_count) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n_rows) return;
  const int32_t c = cluster[i];
  if (wp_checked(c >= 0 && static_cast<size_t>(c) <= i, kSiteNearDup)) atomicAdd(row_count + c, 1u);
}

}  // namespace wp
