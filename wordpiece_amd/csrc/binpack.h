// binpack.h — encoded documents packed into rows by best-fit decreasing on the device (wp_pack_best_fit); the contract
// is include/wordpiece_amd_binpack.h, its Python statement tests/binpack_model.py.  The pieces, their units and the
// write pass are those of packing.h; what is new is the order of the units and the rows they fall into.
//
// Best fit looks sequential: every unit asks for the fullest row that still takes it.  But a unit's row depends only on
// its length and on its rank among the units sorted by length, and the answer for ALL ranks has a run-length form that
// follows from the histogram of the lengths alone (binpack_path.h, binpack_plan_host: work in max_len, not in
// documents).  So the device does the per-piece work and nothing else:
//
//   hist    binpack_hist_kernel: u_k = P[k + 1] - P[k] of every piece into a histogram of L counters, and the sort key
//           L - u_k.  A capped grid walks tiles of kBinTile pieces; a lane owns kBinItems consecutive pieces (five
//           consecutive words of P).  The counters of a workgroup live in LDS (L <= 8192: 32 KB).  Two things keep the
//           LDS atomics off the hot bins: the full unit u == L — every piece but the last of a split document, every
//           truncated one — is counted by a wave ballot, one atomic per wave and item; and a lane folds the run of
//           equal lengths among its own consecutive items into one atomic.  Each workgroup then adds its non-zero bins
//           to the 64-bit device histogram, once.
//   sort    radix_sort_pairs<uint32_t> over the key bits with identity values, stable: sigma, the pieces by length
//           descending and by k ascending inside a length.  The host plans meanwhile.
//   place   binpack_place_kernel: one sigma-rank per lane in tiles of kBinTile.  The ranks of a tile are contiguous, so
//           its runs are a contiguous slice of the run table: thread 0 finds the slice with two searches, the slice goes
//           to LDS where it has at most kBinRunSlice entries (else the lanes search it in global memory), a lane finds
//           its run there and its row's range in the row-range table, and writes the tables of the packed order: P2 at
//           the unit's place in its row, src2 beside it.  All closed forms: no scan, no atomics.
//   rows    binpack_rows_kernel: one lane per row, row_first from the row's range.
//   write   seqpack_write_kernel of packing.h over P2, src2 and row_first, unchanged.
//
// Per piece: 8 B read and 4 B written by hist, the sort's two passes over 8 B pairs, 12 B gathered and 8 B written by
// place.  Every computed index goes through wp_in_bounds (kSitePack): the bounds-checking build also checks that the
// unit a rank holds has the length its run says, i.e. that the sort and the plan agree.
#pragma once
#include "../../include/wordpiece_amd_binpack.h"
#include "packing.h"

namespace wp {

constexpr int kBinItems = 4;
constexpr int kBinTile = kBlock * kBinItems;  // pieces per tile of the hist pass, ranks per tile of the place pass
constexpr int kBinMaxLen = WP_BINPACK_MAX_LEN;
constexpr int kBinRunSlice = 128;             // runs of a tile's slice that LDS holds (5 KB): a tile of real lengths has a few
constexpr unsigned kBinHistGrid = 512;        // workgroups of the hist pass: each ends in a pass of global atomics
static_assert(kBinMaxLen * sizeof(uint32_t) <= 32768, "a workgroup's histogram must fit 32 KB of LDS");

// hist[u] += the pieces of u cells (hist: L + 1 64-bit counters, cleared by the caller); keys[k] = L - u_k.
__global__ __launch_bounds__(kBlock) void binpack_hist_kernel(const uint32_t *__restrict__ P, uint32_t n_p, uint32_t L,
                                                              uint32_t *__restrict__ keys, unsigned long long *__restrict__ hist) {
  __shared__ uint32_t s_hist[kBinMaxLen];  // s_hist[u - 1]
  for (uint32_t b = threadIdx.x; b < L; b += kBlock) s_hist[b] = 0;
  __syncthreads();
  const uint32_t n_tiles = (n_p + kBinTile - 1) / kBinTile;
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint32_t k0 = tile * kBinTile + threadIdx.x * kBinItems;
    uint32_t p_prev = k0 < n_p ? P[k0] : 0u;
    uint32_t run_u = 0, run_n = 0;  // the run of equal lengths among this lane's items so far
#pragma unroll
    for (int j = 0; j < kBinItems; j++) {
      const uint32_t k = k0 + j;
      const bool valid = k < n_p;
      uint32_t u = 0;
      if (valid) {
        const uint32_t p_next = P[k + 1];
        u = p_next - p_prev;
        p_prev = p_next;
      }
      const bool ok = valid && wp_checked(u >= 1 && u <= L, kSitePack);
      if (valid) keys[k] = ok ? L - u : 0u;
      const bool full = ok && u == L;
      const unsigned long long m = __ballot(full);  // (the loops are uniform: every lane of the wave is here)
      if (full && lane_id() == __ffsll(static_cast<long long>(m)) - 1) atomicAdd(&s_hist[L - 1], static_cast<uint32_t>(__popcll(m)));
      if (ok && !full) {
        if (u == run_u) {
          run_n++;
        } else {
          if (run_n) atomicAdd(&s_hist[run_u - 1], run_n);
          run_u = u;
          run_n = 1;
        }
      }
    }
    if (run_n) atomicAdd(&s_hist[run_u - 1], run_n);
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < L; b += kBlock) {
    const uint32_t n = s_hist[b];
    if (n) atomicAdd(&hist[b + 1], static_cast<unsigned long long>(n));
  }
}

// the largest a in [0, n - 1] with tab[a].first_rank <= i (tab[0].first_rank == 0; n >= 1)
__device__ __forceinline__ uint32_t binpack_run_of(const wp_binpack_run *tab, uint32_t n, uint32_t i) {
  uint32_t a = 0, b = n - 1;
  while (a < b) {
    const uint32_t mid = (a + b + 1) >> 1;
    if (tab[mid].first_rank <= static_cast<long long>(i)) {
      a = mid;
    } else {
      b = mid - 1;
    }
  }
  return a;
}
// the largest a in [0, n - 1] with ranges[a].row0 <= row (ranges[0].row0 == 0; n >= 1)
__device__ __forceinline__ uint32_t binpack_range_of(const wp_binpack_row_range *__restrict__ ranges, uint32_t n, uint32_t row) {
  uint32_t a = 0, b = n - 1;
  while (a < b) {
    const uint32_t mid = (a + b + 1) >> 1;
    if (ranges[mid].row0 <= static_cast<long long>(row)) {
      a = mid;
    } else {
      b = mid - 1;
    }
  }
  return a;
}

// One sigma-rank per lane.  Grid: cdiv(n_p, kBinTile).  sigma[i]: the piece at rank i.  P2[n_p + 1], src2[n_p]: P and
// src0 of the units in packed order, rows back to back.  (All values fit 31 bits: the host checked the totals.)
__global__ __launch_bounds__(kBlock) void binpack_place_kernel(const uint32_t *__restrict__ sigma, const uint32_t *__restrict__ P,
                                                               const int32_t *__restrict__ src0, const wp_binpack_run *__restrict__ runs,
                                                               uint32_t n_runs, const wp_binpack_row_range *__restrict__ ranges,
                                                               uint32_t n_ranges, uint32_t n_p, uint32_t N, uint32_t *__restrict__ P2,
                                                               int32_t *__restrict__ src2) {
  __shared__ wp_binpack_run s_runs[kBinRunSlice];
  __shared__ uint32_t s_slice[2];
  const uint32_t i0 = blockIdx.x * kBinTile, i1 = min(i0 + static_cast<uint32_t>(kBinTile), n_p) - 1;  // the tile's first and last rank
  if (threadIdx.x == 0) {
    const uint32_t lo = binpack_run_of(runs, n_runs, i0);
    s_slice[0] = lo;
    s_slice[1] = lo + binpack_run_of(runs + lo, n_runs - lo, i1);
    if (blockIdx.x == 0) P2[n_p] = N;
  }
  __syncthreads();
  const uint32_t lo = s_slice[0], n_slice = s_slice[1] - lo + 1;
  const bool in_lds = n_slice <= static_cast<uint32_t>(kBinRunSlice);
  if (in_lds) {
    for (uint32_t t = threadIdx.x; t < n_slice; t += kBlock) s_runs[t] = runs[lo + t];
  }
  __syncthreads();
  const wp_binpack_run *tab = in_lds ? s_runs : runs + lo;
#pragma unroll
  for (int j = 0; j < kBinItems; j++) {
    const uint32_t i = i0 + j * kBlock + threadIdx.x;
    if (i > i1) continue;
    const wp_binpack_run r = tab[binpack_run_of(tab, n_slice, i)];
    const uint32_t per = static_cast<uint32_t>(r.per_row), d = i - static_cast<uint32_t>(r.first_rank);
    const uint32_t piece = sigma[i];
    bool ok = per >= 1 && r.first_rank <= static_cast<long long>(i) && piece < n_p;
    const uint32_t jr = ok ? d / per : 0u, t = d - jr * per;
    ok = ok && static_cast<long long>(jr) < r.n_rows;
#ifdef WP_DEBUG_BOUNDS
    ok = ok && P[piece + 1] - P[piece] == static_cast<uint32_t>(r.unit);  // the sort and the plan agree on this rank's length
#endif
    if (!wp_checked(ok, kSitePack)) continue;
    const uint32_t row = static_cast<uint32_t>(r.row0) + jr;
    const wp_binpack_row_range g = ranges[binpack_range_of(ranges, n_ranges, row)];
    const uint32_t dr = row - static_cast<uint32_t>(g.row0);
    const uint32_t k2 = static_cast<uint32_t>(g.first_unit) + dr * static_cast<uint32_t>(g.units_per_row) + static_cast<uint32_t>(r.slot0) + t;
    const bool in = g.row0 <= static_cast<long long>(row) && static_cast<long long>(dr) < g.n_rows && k2 < n_p;
    if (!wp_checked(in, kSitePack)) continue;
    P2[k2] = static_cast<uint32_t>(g.first_cell) + dr * static_cast<uint32_t>(g.cells_per_row) + static_cast<uint32_t>(r.col0) +
             t * static_cast<uint32_t>(r.unit);
    src2[k2] = src0[piece];
  }
}

// One lane per row, and one for the entry behind the last: row_first[row] = the first unit of the row in packed order,
// row_first[n_out] = n_p.  (n_out <= n_p: row_first has n_p + 1 entries.)
__global__ __launch_bounds__(kBlock) void binpack_rows_kernel(const wp_binpack_row_range *__restrict__ ranges, uint32_t n_ranges,
                                                              uint32_t n_out, uint32_t n_p, uint32_t *__restrict__ row_first) {
  const uint32_t row = blockIdx.x * kBlock + threadIdx.x;
  if (row > n_out) return;
  uint32_t first = n_p;
  if (row < n_out) {
    const wp_binpack_row_range g = ranges[binpack_range_of(ranges, n_ranges, row)];
    const uint32_t dr = row - static_cast<uint32_t>(g.row0);
    first = static_cast<uint32_t>(g.first_unit) + dr * static_cast<uint32_t>(g.units_per_row);
    if (!wp_checked(g.row0 <= static_cast<long long>(row) && static_cast<long long>(dr) < g.n_rows && first < n_p, kSitePack)) return;
  }
  row_first[row] = first;
}

}  // namespace wp
