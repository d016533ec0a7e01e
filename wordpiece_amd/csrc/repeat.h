// repeat.h — the kernels of the repeated-span search (include/wordpiece_amd.h, section "repeated spans"; host path:
// repeat_path.h).  One ragged batch checked against itself.  The windows, their keys, the one stable sort of (key, flat
// position), the runs, the head comparison and the representative of every member are the n-gram overlap's (overlap.h,
// included from here: nothing is copied): since the sort is stable the positions ascend inside a run, so the
// representative — the first member of the run that holds the same bytes — is the first occurrence of the window.
//   Back to the elements.  Every sorted member stores the flat position of its first occurrence at its own flat
// position: one lane per position, no atomics.  A position without a window keeps kRepNone.
//   Flags.  A tile of kRepTile elements per workgroup: the rows of its first and last element once, then every lane finds
// its row within that range, as the key kernel does.  A window is a repeat where its first occurrence is not itself and,
// at scope 1, lies in front of the start of its row.  H = the exclusive scan of the flags.
//   Cover.  The same tiles with H of the tile and of a halo of kRepHalo elements in front of it in LDS: element e is
// covered iff H[e + 1] != H[max(row start, e - k + 1)], no loop over k.  The repeat with H[e] == H[row start] is the
// first of its row and stores the row's first_repeat and its source; the row of the source is the one bisection over
// all rows that is left, at most one per row.  C = the exclusive scan of the cover flags: a kept element e goes to
// e - C[e] of the cut, which is the exclusive scan of the keep flags without a second scan, and row i of the cut begins
// at row start - C[row start].
//   Cut.  Ids are stored directly.  Bytes go through LDS: a workgroup compacts its kRepCutTile bytes at (position -
// position of the tile's first kept byte), in the byte phase of the output, and stores whole aligned words; the at most
// two words it shares with its neighbours are written byte by byte.  No byte is written twice and no value depends on
// an order of execution.
#pragma once
// overlap.h wholesale, and group.h through it: the window keys, the list, the head comparison, the representatives, the
// per-row results, the kept rows, ovl_row_of
#include "overlap.h"

namespace wp {

constexpr int kRepTile = 2048;                          // elements per workgroup of the flag and the cover kernel
constexpr int kRepHalo = kOvlMaxNgram;                  // elements in front of a tile whose H the cover kernel holds (k - 1 at most)
constexpr int kRepCutWords = 4;                         // input words a lane of the byte cut takes
constexpr int kRepCutTile = kBlock * 4 * kRepCutWords;  // bytes per workgroup of the byte cut
constexpr uint32_t kRepNone = 0xffffffffu;              // first[e] of a position without a window
static_assert(kRepHalo >= kOvlMaxNgram - 1, "the windows that cover the first element of a tile begin inside the halo");

// the counters of a call, 64 bits each, in d_scalars from kScalarRep on (the overlap kernels count into the same places)
enum RepCounter { kRepRepeatRows = 0, kRepCollided = 1, kRepCounters = 4 };
static_assert(int(kRepRepeatRows) == int(kOvlHitRows) && int(kRepCollided) == int(kOvlCollided),"ovl_row_results_kernel and ovl_ref_head_kernel count here");

// Sorted position s of the m windows (val: their flat positions, rep: the first member of the run with the same bytes):
// first[its flat position] = the flat position of that member, the first occurrence.  first starts as kRepNone.
__global__ __launch_bounds__(kBlock) void rep_back_kernel(const uint32_t *__restrict__ val, const uint32_t *__restrict__ rep, size_t m, size_t n_elems,
                                                          uint32_t *__restrict__ first) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s >= m) return;
  const uint32_t rp = rep[s];
  if (!wp_checked(rp <= s, kSiteRepeat)) return;
  const uint32_t p = val[s], q = val[rp];
  if (wp_checked(p < n_elems && q <= p, kSiteRepeat)) first[p] = q;
}

// the rows of the first and of the last element of the tile that begins at `base`, by two waves, into s_rows
__device__ __forceinline__ void rep_tile_rows(const uint32_t *__restrict__ byte_off, size_t n_rows, size_t base, size_t n_elems, uint32_t elem_bytes,
                                              uint32_t *s_rows) {
  const int tid = threadIdx.x;
  if (tid == 0 || tid == kWave) {
    const size_t e = tid == 0 ? base : min(base + kRepTile, n_elems) - 1;
    s_rows[tid != 0] = ovl_row_of(byte_off, 0, static_cast<uint32_t>(n_rows - 1), e * elem_bytes);
  }
  __syncthreads();
}

// Tile blockIdx.x of the elements: hit[e] = 1 where the window at e is a repeat (scope 1: its first occurrence lies in
// front of its row, which only a window that occurred before has to look up); src (optional) = the first occurrence of
// a repeat, else -1.
__global__ __launch_bounds__(kBlock) void rep_flag_kernel(const uint32_t *__restrict__ first, const uint32_t *__restrict__ byte_off, size_t n_rows,
                                                          size_t n_elems, uint32_t elem_bytes, uint32_t scope, uint32_t *__restrict__ hit,
                                                          long long *__restrict__ src) {
  __shared__ uint32_t s_rows[2];
  const size_t base = static_cast<size_t>(blockIdx.x) * kRepTile;
  rep_tile_rows(byte_off, n_rows, base, n_elems, elem_bytes, s_rows);
  const uint32_t r_lo = s_rows[0], r_hi = s_rows[1];
  for (int p = threadIdx.x; p < kRepTile; p += kBlock) {
    const size_t e = base + p;
    if (e >= n_elems) break;
    const uint32_t f = first[e];
    bool h = f != kRepNone && f != e;
    if (h && (!wp_in_bounds(f < e, kSiteRepeat) || f > e)) h = false;
    if (h && scope != 0) {
      const uint32_t r = ovl_row_of(byte_off, r_lo, r_hi, e * elem_bytes);
      h = static_cast<size_t>(f) * elem_bytes < byte_off[r];
    }
    hit[e] = h ? 1u : 0u;
    if (src) src[e] = h ? static_cast<long long>(f) : -1ll;
  }
}

// Tile blockIdx.x of the elements (H: the exclusive scan of hit over n_elems + 1 entries): cover[e] = 1 where a repeat
// window of its row holds e, mask[e] the same as a byte (optional).  The repeat that is the first of its row stores
// first_repeat, first_src_row and first_src_pos of the row (they start as -1).
__global__ __launch_bounds__(kBlock) void rep_cover_kernel(const uint32_t *__restrict__ hit, const uint32_t *__restrict__ H,
                                                           const uint32_t *__restrict__ first, const uint32_t *__restrict__ byte_off, size_t n_rows,
                                                           size_t n_elems, uint32_t elem_bytes, uint32_t k, uint32_t *__restrict__ cover,
                                                           uint8_t *__restrict__ mask, long long *__restrict__ first_repeat,
                                                           int32_t *__restrict__ first_src_row, long long *__restrict__ first_src_pos) {
  __shared__ uint32_t s_rows[2];
  __shared__ uint32_t s_H[kRepHalo + kRepTile + 1];
  const size_t base = static_cast<size_t>(blockIdx.x) * kRepTile;
  const size_t lo = base >= kRepHalo ? base - kRepHalo : 0;
  for (int t = threadIdx.x; t < kRepHalo + kRepTile + 1; t += kBlock) s_H[t] = lo + t <= n_elems ? H[lo + t] : 0u;
  rep_tile_rows(byte_off, n_rows, base, n_elems, elem_bytes, s_rows);  // (its barrier closes the loads too)
  const uint32_t r_lo = s_rows[0], r_hi = s_rows[1];
  for (int p = threadIdx.x; p < kRepTile; p += kBlock) {
    const size_t e = base + p;
    if (e >= n_elems) break;
    const uint32_t r = ovl_row_of(byte_off, r_lo, r_hi, e * elem_bytes);
    const size_t s = byte_off[r] / elem_bytes;
    const size_t from = e + 1 >= s + k ? e + 1 - k : s;
    const bool inside = s <= e && from >= lo;
    uint32_t cov = 0;
    if (wp_checked(inside, kSiteRepeat)) cov = s_H[e + 1 - lo] != s_H[from - lo] ? 1u : 0u;
    cover[e] = cov;
    if (mask) mask[e] = static_cast<uint8_t>(cov);
    if (inside && hit[e] && s_H[e - lo] == H[s]) {
      first_repeat[r] = static_cast<long long>(e - s);
      const uint32_t f = first[e];
      if (wp_checked(f < e, kSiteRepeat)) {
        const uint32_t fr = ovl_row_of(byte_off, 0, static_cast<uint32_t>(n_rows - 1), static_cast<size_t>(f) * elem_bytes);
        first_src_row[r] = static_cast<int32_t>(fr);
        first_src_pos[r] = static_cast<long long>(f) - static_cast<long long>(byte_off[fr] / elem_bytes);
      }
    }
  }
}

// Row i of the cut (C: the exclusive scan of cover over n_elems + 1 entries): cut_off[i] = the kept elements in front of
// the row; entry n_rows closes the offsets with their number.
__global__ __launch_bounds__(kBlock) void rep_cut_off_kernel(const uint32_t *__restrict__ Cv, const uint32_t *__restrict__ byte_off, size_t n_rows,
                                                             size_t n_elems, uint32_t elem_bytes, long long *__restrict__ cut_off) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i > n_rows) return;
  const size_t a = byte_off[i] / elem_bytes;
  if (!wp_checked(a <= n_elems, kSiteRepeat)) return;
  cut_off[i] = static_cast<long long>(a) - static_cast<long long>(Cv[a]);
}

// The cut of ids: a kept element e goes to e - C[e]
__global__ __launch_bounds__(kBlock) void rep_cut_ids_kernel(const uint32_t *__restrict__ d32, const uint32_t *__restrict__ cover,
                                                             const uint32_t *__restrict__ Cv, size_t n_elems, uint32_t *__restrict__ out) {
  const size_t e = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= n_elems || cover[e]) return;
  const uint32_t c = Cv[e];
  if (wp_checked(c <= e, kSiteRepeat)) out[e - c] = d32[e];
}

// The cut of bytes, tile blockIdx.x of kRepCutTile bytes.  Its kept bytes are [o0, o1) of the output.  A lane takes
// whole input words and puts their kept bytes into LDS at (output position - the word boundary at or below o0), so LDS
// word j is output word o0 / 4 + j; then the words inside [o0, o1) are stored whole and the bytes of the first and the
// last word, which the neighbouring tiles share, one by one.
__global__ __launch_bounds__(kBlock) void rep_cut_bytes_kernel(const uint32_t *__restrict__ d32, const uint32_t *__restrict__ cover,
                                                               const uint32_t *__restrict__ Cv, size_t n_elems, size_t cap, uint32_t *__restrict__ out) {
  __shared__ uint32_t s_out[kRepCutTile / 4 + 2];
  uint8_t *sb = reinterpret_cast<uint8_t *>(s_out);
  const size_t base = static_cast<size_t>(blockIdx.x) * kRepCutTile;
  const size_t end = min(base + kRepCutTile, n_elems);
  const size_t c0 = Cv[base], c1 = Cv[end];
  const bool sane = c0 <= base && c1 <= end && c0 <= c1 && c1 - c0 <= end - base && end - c1 <= cap;
  if (!wp_checked(sane, kSiteRepeat)) return;  // (the whole workgroup leaves together)
  const size_t o0 = base - c0, o1 = end - c1, w0 = o0 & ~static_cast<size_t>(3);
#pragma unroll
  for (int it = 0; it < kRepCutWords; it++) {
    const size_t e0 = base + 4 * (static_cast<size_t>(it) * kBlock + threadIdx.x);
    if (e0 >= end) continue;
    const uint32_t x = d32[e0 >> 2];
    size_t o = e0 - Cv[e0];
    for (uint32_t b = 0; b < 4 && e0 + b < end; b++) {
      if (cover[e0 + b]) continue;
      const size_t at = o - w0;
      if (wp_checked(o >= o0 && at < kRepCutTile + 4, kSiteRepeat)) sb[at] = static_cast<uint8_t>(x >> (8u * b));
      o++;
    }
  }
  __syncthreads();
  uint8_t *out8 = reinterpret_cast<uint8_t *>(out);
  const size_t words = (o1 - w0 + 3) >> 2;
  for (size_t j = threadIdx.x; j < words; j += kBlock) {
    const size_t at = w0 + 4 * j;
    if (at >= o0 && at + 4 <= o1) {
      out[at >> 2] = s_out[j];
    } else {
      for (uint32_t b = 0; b < 4; b++) {
        if (at + b >= o0 && at + b < o1) out8[at + b] = sb[4 * j + b];
      }
    }
  }
}

}  // namespace wp
