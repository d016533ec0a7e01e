// overlap.h — the kernels of the n-gram overlap search (include/wordpiece_amd.h, section "n-gram overlap"; host path:
// overlap_path.h).  Two ragged batches, the corpus and the reference set, as dedup takes them.  Everything is flat over
// the elements of a batch: a position finds its row by bisection in the byte offsets, so one row of 10^8 elements costs
// what 10^6 rows of 100 do and no lane, wave or workgroup walks a row.
//   Window keys.  The key of the window of k elements at flat position p is M(sum_{t<k} m(x[p+t]) B^(k-1-t)) mod 2^64,
// m(x) = (x + 1) G.  A workgroup takes kOvlSpan elements, a tile of kOvlTile positions and a halo, through LDS, scans
// the Horner prefixes Q[j] = Q[j-1] B + m(x[j-1]) (a linear recurrence: a scan step over d threads multiplies by a
// power of B the host hands in), and every window key is Q[p+k] - Q[p] B^k: O(1) per window whatever k is.  A window
// counts where it ends inside the row of its first element.  The same kernel serves both batches: for the reference
// set it stores keys, for the corpus it looks every key up and stores candidates.
//   Table.  The valid reference windows are sorted stably as (narrowed key, flat position); in a run of equal keys
// every member is compared with the head byte by byte, and the members that differ with the differing members in front
// of them, so that every member knows the first member equal to it: its representative.  The representatives are the
// table entries, in sorted order; a bucket index over the top bits of the narrowed key holds [first, last) of its
// entries in two adjacent words.
//   Lookup.  One lane per corpus window: bucket, lower bound, and a candidate where the key is there.  The candidates
// are compacted and compared with the entries of their key, in order, by groups of kOvlLanes lanes; an equal entry makes
// the position a hit and marks the entry.  Since entries ascend in position, the first equal entry is the smallest
// reference row that holds the window.
//   Results.  H = the exclusive scan of the hit flags: hits of a row are a difference of H at its ends, element e is
// covered iff H[e + 1] - H[max(row start, e - k + 1)] > 0, the first hit of a row is the hit with H[e] == H[row start].
// Nothing is an atomic on a result; the counters are integer sums.
#pragma once
#include "common.h"
#include "group.h"  // mix64, word_at, same_words, last_le, run_of, ragged_row; the round and compact-form kernels run beside these

namespace wp {

constexpr int kOvlMaxNgram = 64;                      // elements of a window, at most
constexpr int kOvlItems = 5;                          // elements a lane of the key kernel scans
constexpr int kOvlSpan = kBlock * kOvlItems;          // elements a workgroup of the key kernel reads
constexpr int kOvlTile = 1216;                        // T: window positions per workgroup of the key kernel
constexpr int kOvlLanes = 16;                         // lanes that compare one candidate with a table entry
constexpr int kOvlMaxBucketBits = 26;
constexpr uint64_t kOvlB = kGolden;                   // B (odd)
constexpr uint64_t kOvlG = 0xd6e8feb86659fd93ull;     // G (odd)
static_assert(kOvlTile + kOvlMaxNgram <= kOvlSpan, "the halo of the last position of a tile lies inside the span");

// the counters of a call, 64 bits each, in d_scalars from kScalarOvl on
enum OvlCounter { kOvlHitRows = 0, kOvlCollided = 1, kOvlCounters = 4 };

// the powers of B the key kernel multiplies by
struct OvlPowers {
  uint64_t step[6];  // B^(kOvlItems * 2^i): the wave scan over 2^i lanes
  uint64_t wave;     // B^(kOvlItems * kWave)
  uint64_t bk;       // B^k
};

// Row i of a batch through ragged_row (offsets checked, byte_off, *n_elems).  *n_windows: the windows of the batch,
// summed per wave.
__global__ __launch_bounds__(kBlock) void ovl_rows_kernel(const long long *__restrict__ row_off, size_t n_rows, uint32_t elem_bytes, uint32_t k,
                                                          uint32_t *__restrict__ byte_off, uint32_t *__restrict__ bad,
                                                          unsigned long long *__restrict__ n_elems, unsigned long long *__restrict__ n_windows) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  unsigned long long w = 0;
  if (i <= n_rows) {
    const RaggedRow r = ragged_row(row_off, n_rows, elem_bytes, i, byte_off, bad, n_elems);
    if (r.row && r.len >= k) w = r.len - k + 1;
  }
  w = wave_reduce_sum64(w);
  if (lane_id() == 0 && w != 0) atomicAdd(n_windows, w);
}

// the last r in [lo, hi] with byte_off[r] <= addr (byte_off[lo] <= addr): the row that holds the byte, empty rows passed
__device__ __forceinline__ uint32_t ovl_row_of(const uint32_t *__restrict__ byte_off, uint32_t lo, uint32_t hi, size_t addr) {
  return last_le(byte_off, lo, hi + 1u, addr);
}

// element e of the data (e < n_elems): a byte or an id, read as part of its aligned word
__device__ __forceinline__ uint32_t ovl_elem(const uint32_t *__restrict__ d32, size_t e, uint32_t elem_bytes) {
  if (elem_bytes == 4) return d32[e];
  return (d32[e >> 2] >> (8u * static_cast<uint32_t>(e & 3u))) & 0xffu;
}

// Tile blockIdx.x of the positions [0, n_elems) of a batch of n_rows >= 1 rows.  The span goes through LDS, lane t scans
// its kOvlItems elements, the wave and the workgroup combine the lanes' values, and Q[0 .. kOvlSpan] is in LDS; then one
// lane per position of the tile, striped: its row within the rows of the tile, whether the window fits the row, its key.
// ent_key == nullptr (the reference set): key_out[e] = the key narrowed to `mask`, valid[e] = 1 where position e has a
// window; valid[n_elems] = 0 closes the flags for their scan.  Otherwise (the corpus): the key's bucket (bucket: two
// words per bucket, [first, last) in the entries; shift: the narrowed key's bits below the bucket number), the lower
// bound of the key among the bucket's entries, and valid[e] = 1, ent_out[e] = that entry where its key is the same: a
// candidate.  utf8 != 0 (bytes; the repeat layer, repeat.h — the overlap call passes 0): a window also has to begin at a
// byte that is no continuation byte and to end in front of one that is none, or at the end of its row.
__global__ __launch_bounds__(kBlock) void ovl_keys_kernel(const uint32_t *__restrict__ d32, size_t n_elems, const uint32_t *__restrict__ byte_off,
                                                          size_t n_rows, uint32_t elem_bytes, uint32_t k, OvlPowers pw, uint64_t mask,
                                                          uint64_t *__restrict__ key_out, uint32_t *__restrict__ valid,
                                                          const uint64_t *__restrict__ ent_key, const uint32_t *__restrict__ n_ent_dev,
                                                          const uint32_t *__restrict__ bucket, uint32_t shift, size_t n_buckets,
                                                          uint32_t *__restrict__ ent_out, uint32_t utf8) {
  __shared__ uint32_t s_x[kOvlSpan];
  __shared__ uint64_t s_q[kOvlSpan + 1];
  __shared__ uint64_t s_wave[kBlock / kWave];
  __shared__ uint32_t s_rows[2];
  const size_t base = static_cast<size_t>(blockIdx.x) * kOvlTile;
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  for (int t = tid; t < kOvlSpan; t += kBlock) s_x[t] = base + t < n_elems ? ovl_elem(d32, base + t, elem_bytes) : 0u;
  if (tid == 0 || tid == kWave) {  // the rows of the first and of the last position of the tile, by two waves
    const size_t e = tid == 0 ? base : min(base + kOvlTile, n_elems) - 1;
    s_rows[tid != 0] = ovl_row_of(byte_off, 0, static_cast<uint32_t>(n_rows - 1), e * elem_bytes);
  }
  if (blockIdx.x == 0 && tid == 0 && !ent_key) valid[n_elems] = 0;
  __syncthreads();
  // Horner over the lane's elements: h[i] = the value of its first i + 1 elements
  unsigned long long h[kOvlItems], acc = 0;
#pragma unroll
  for (int i = 0; i < kOvlItems; i++) {
    acc = acc * kOvlB + (static_cast<unsigned long long>(s_x[tid * kOvlItems + i]) + 1ull) * kOvlG;
    h[i] = acc;
  }
  // inclusive scan over the wave, every value scaled to the end of its lane's elements: the value d lanes back has
  // kOvlItems * d elements behind it
  unsigned long long v = acc;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const unsigned long long t = __shfl_up(v, 1 << i, kWave);
    if (lane >= (1 << i)) v += t * pw.step[i];
  }
  if (lane == kWave - 1) s_wave[w] = v;
  const unsigned long long prev = __shfl_up(v, 1, kWave);
  __syncthreads();
  unsigned long long carry = 0;  // the waves in front of this one, scaled to its first element
  for (int i = 0; i < w; i++) carry = carry * pw.wave + s_wave[i];
  // Q at the lane's first element: the waves in front pass the lanes in front (B^(kOvlItems * lane)), which are added
  unsigned long long lanes_pow = 1, p5 = pw.step[0];
  for (int b = lane; b != 0; b >>= 1, p5 *= p5) {
    if (b & 1) lanes_pow *= p5;
  }
  const unsigned long long q = carry * lanes_pow + (lane == 0 ? 0ull : prev);
  if (tid == 0) s_q[0] = 0;
  unsigned long long bi = kOvlB;
#pragma unroll
  for (int i = 0; i < kOvlItems; i++) {
    s_q[tid * kOvlItems + i + 1] = q * bi + h[i];
    bi *= kOvlB;
  }
  __syncthreads();
  const uint32_t r_lo = s_rows[0], r_hi = s_rows[1];
  const uint32_t n_ent = ent_key ? *n_ent_dev : 0u;
  const size_t win_bytes = static_cast<size_t>(k) * elem_bytes;
  for (int p = tid; p < kOvlTile; p += kBlock) {
    const size_t e = base + p;
    if (e >= n_elems) break;
    const size_t addr = e * elem_bytes;
    const uint32_t r = ovl_row_of(byte_off, r_lo, r_hi, addr);
    bool fits = addr + win_bytes <= byte_off[r + 1];
    if (utf8 && fits) fits = (s_x[p] & 0xc0u) != 0x80u && (addr + win_bytes == byte_off[r + 1] || (s_x[p + k] & 0xc0u) != 0x80u);
    const uint64_t key = mix64(s_q[p + k] - s_q[p] * pw.bk) & mask;
    if (!ent_key) {
      key_out[e] = key;
      valid[e] = fits ? 1u : 0u;
      continue;
    }
    uint32_t cand = 0, ent = 0;
    const size_t b = static_cast<size_t>(key >> shift);
    if (fits && wp_checked(b < n_buckets, kSiteOverlap)) {
      uint32_t lo = bucket[2 * b], hi = bucket[2 * b + 1];
      if (wp_checked(lo <= hi && hi <= n_ent, kSiteOverlap)) {
        const uint32_t end = hi;
        while (lo < hi) {  // the first entry of the bucket whose key is not below this one
          const uint32_t mid = lo + ((hi - lo) >> 1);
          if (ent_key[mid] < key) lo = mid + 1; else hi = mid;
        }
        if (lo < end && ent_key[lo] == key) {
          cand = 1;
          ent = lo;
        }
      }
    }
    valid[e] = cand;
    ent_out[e] = ent;
  }
}

// The valid windows of the reference set, in order: k0[j] = the key, v0[j] = the flat position (pos: the exclusive scan
// of valid)
__global__ __launch_bounds__(kBlock) void ovl_list_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ valid,
                                                          const uint32_t *__restrict__ pos, size_t n_elems, size_t m, uint64_t *__restrict__ k0,
                                                          uint32_t *__restrict__ v0) {
  const size_t e = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= n_elems || !valid[e]) return;
  const uint32_t j = pos[e];
  if (wp_checked(j < m, kSiteOverlap)) {
    k0[j] = key[e];
    v0[j] = static_cast<uint32_t>(e);
  }
}

// Sorted position s of the m reference windows (val: their flat positions): differ[s] = 1 where the window is not the
// one of its run's head.  Heads, and so the runs of one member, read nothing.
__global__ __launch_bounds__(kBlock) void ovl_ref_head_kernel(const uint32_t *__restrict__ d32, size_t n_bytes, const uint32_t *__restrict__ val,
                                                              const uint32_t *__restrict__ head, const uint32_t *__restrict__ run,
                                                              const uint32_t *__restrict__ head_pos, size_t m, uint32_t elem_bytes, uint32_t k,
                                                              uint32_t *__restrict__ differ, unsigned long long *__restrict__ counters) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  uint32_t d = 0;
  if (s < m) {
    const uint32_t r = run_of(head, run, s);
    if (wp_checked(r < m, kSiteOverlap)) {
      const uint32_t hs = head_pos[r];
      const uint32_t wb = k * elem_bytes;
      if (hs != s && wp_checked(hs < s, kSiteOverlap)) {
        const size_t a = static_cast<size_t>(val[s]) * elem_bytes, b = static_cast<size_t>(val[hs]) * elem_bytes;
        if (wp_checked(a + wb <= n_bytes && b + wb <= n_bytes, kSiteOverlap)) d = same_words(d32, a, d32, b, wb) ? 0u : 1u;
      }
    }
    differ[s] = d;
  }
  d = wave_reduce_sum(d);
  if (lane_id() == 0 && d != 0) atomicAdd(counters + kOvlCollided, static_cast<unsigned long long>(d));
}

// Sorted position s: rep[s] = the first member of its run that holds the same window — the head where differ[s] == 0,
// else the first differing member in front of s that equals it, else s itself.  entry[s] = 1 where rep[s] == s;
// entry[m] = 0 closes the flags for their scan.  A run is longer than its duplicates only under a key collision, so at
// 64 bits the second scan reads nothing.
__global__ __launch_bounds__(kBlock) void ovl_ref_rep_kernel(const uint32_t *__restrict__ d32, size_t n_bytes, const uint32_t *__restrict__ val,
                                                             const uint32_t *__restrict__ head, const uint32_t *__restrict__ run,
                                                             const uint32_t *__restrict__ head_pos, const uint32_t *__restrict__ differ, size_t m,
                                                             uint32_t elem_bytes, uint32_t k, uint32_t *__restrict__ rep, uint32_t *__restrict__ entry) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s == 0) entry[m] = 0;
  if (s >= m) return;
  uint32_t rp = static_cast<uint32_t>(s);
  const uint32_t r = run_of(head, run, s);
  if (wp_checked(r < m, kSiteOverlap)) {
    const uint32_t hs = head_pos[r];
    if (wp_checked(hs <= s, kSiteOverlap)) {
      if (!differ[s]) {
        rp = hs;
      } else {
        const uint32_t wb = k * elem_bytes;
        const size_t a = static_cast<size_t>(val[s]) * elem_bytes;
        for (uint32_t t = hs + 1; t < s; t++) {
          if (!differ[t]) continue;
          const size_t b = static_cast<size_t>(val[t]) * elem_bytes;
          if (wp_checked(a + wb <= n_bytes && b + wb <= n_bytes, kSiteOverlap) && same_words(d32, a, d32, b, wb)) {
            rp = t;
            break;
          }
        }
      }
    }
  }
  rep[s] = rp;
  entry[s] = rp == s ? 1u : 0u;
}

// Sorted position s: ent_of[s] = the table entry of its window (entry_pos: the exclusive scan of entry); an entry takes
// its key and its flat position, and its mark starts at 0.
__global__ __launch_bounds__(kBlock) void ovl_table_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                           const uint32_t *__restrict__ rep, const uint32_t *__restrict__ entry_pos, size_t m,
                                                           uint32_t *__restrict__ ent_of, uint64_t *__restrict__ ent_key,
                                                           uint32_t *__restrict__ ent_pos, uint32_t *__restrict__ ent_hit) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s >= m) return;
  const uint32_t rp = rep[s];
  if (!wp_checked(rp <= s, kSiteOverlap)) return;
  const uint32_t t = entry_pos[rp];
  if (!wp_checked(t < m, kSiteOverlap)) return;
  ent_of[s] = t;
  if (rp == s) {
    ent_key[t] = key[s];
    ent_pos[t] = val[s];
    ent_hit[t] = 0;
  }
}

// Entry t: the first entry of its bucket stores the bucket's first word, the last one its second (the index starts as
// zeros: an empty bucket is [0, 0))
__global__ __launch_bounds__(kBlock) void ovl_bucket_kernel(const uint64_t *__restrict__ ent_key, const uint32_t *__restrict__ n_ent_dev, size_t m,
                                                            uint32_t shift, size_t n_buckets, uint32_t *__restrict__ bucket) {
  const size_t t = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  const size_t n_ent = min(static_cast<size_t>(*n_ent_dev), m);
  if (t >= n_ent) return;
  const size_t b = static_cast<size_t>(ent_key[t] >> shift);
  if (!wp_checked(b < n_buckets, kSiteOverlap)) return;
  if (t == 0 || static_cast<size_t>(ent_key[t - 1] >> shift) != b) bucket[2 * b] = static_cast<uint32_t>(t);
  if (t + 1 == n_ent || static_cast<size_t>(ent_key[t + 1] >> shift) != b) bucket[2 * b + 1] = static_cast<uint32_t>(t + 1);
}

// Candidate c by a group of kOvlLanes lanes and coalesced reads: the corpus window at cand_e[c] against the entries of
// its key from cand_t[c] on, in order, until one is equal.  Then hit[e] = 1, ent_at[e] = that entry, and the entry is
// marked (every writer stores the same 1).
__global__ __launch_bounds__(kBlock) void ovl_verify_kernel(const uint32_t *__restrict__ c32, size_t n_bytes, const uint32_t *__restrict__ r32,
                                                            size_t n_ref_bytes, const uint32_t *__restrict__ cand_e,
                                                            const uint32_t *__restrict__ cand_t, size_t n_cand, const uint64_t *__restrict__ ent_key,
                                                            const uint32_t *__restrict__ ent_pos, const uint32_t *__restrict__ n_ent_dev,
                                                            size_t m, uint32_t elem_bytes, uint32_t k, uint32_t *__restrict__ hit,
                                                            uint32_t *__restrict__ ent_at, uint32_t *__restrict__ ent_hit) {
  const size_t c = (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x) / kOvlLanes;
  const uint32_t sub = threadIdx.x % kOvlLanes;
  if (c >= n_cand) return;  // (a whole group leaves together)
  const size_t n_ent = min(static_cast<size_t>(*n_ent_dev), m);
  const uint32_t e = cand_e[c], t0 = cand_t[c];
  const uint32_t wb = k * elem_bytes, words = (wb + 3u) >> 2;
  const size_t a = static_cast<size_t>(e) * elem_bytes;
  if (!wp_checked(t0 < n_ent && a + wb <= n_bytes, kSiteOverlap)) return;
  const uint64_t key = ent_key[t0];
  for (size_t t = t0; t < n_ent && ent_key[t] == key; t++) {
    const size_t b = static_cast<size_t>(ent_pos[t]) * elem_bytes;
    const bool inside = b + wb <= n_ref_bytes;
    uint32_t differ = wp_checked(inside, kSiteOverlap) ? 0u : 1u;
    if (inside) {
      for (uint32_t i = sub; i < words && !differ; i += kOvlLanes) differ = word_at(c32, a, a + wb, i) != word_at(r32, b, b + wb, i) ? 1u : 0u;
    }
#pragma unroll
    for (int d = kOvlLanes / 2; d > 0; d >>= 1) differ |= __shfl_xor(differ, d, kWave);
    if (!differ) {
      if (sub == 0) {
        hit[e] = 1u;
        ent_at[e] = static_cast<uint32_t>(t);
        ent_hit[t] = 1u;
      }
      return;
    }
  }
}

// Element e of the corpus (H: the exclusive scan of hit over n_elems + 1 entries): cover[e] = 1 where a hitting window
// holds it, mask[e] the same as a byte (optional); cover[n_elems] = 0 closes the flags.  The hit that is the first of its
// row stores the row's first_hit and first_ref: the row of the reference set that holds the entry's position.
__global__ __launch_bounds__(kBlock) void ovl_cover_kernel(const uint32_t *__restrict__ hit, const uint32_t *__restrict__ H,
                                                           const uint32_t *__restrict__ ent_at, const uint32_t *__restrict__ ent_pos, size_t m,
                                                           const uint32_t *__restrict__ byte_off, size_t n_rows,
                                                           const uint32_t *__restrict__ ref_byte_off, size_t n_ref, size_t n_elems,
                                                           uint32_t elem_bytes, uint32_t k, uint32_t *__restrict__ cover, uint8_t *__restrict__ mask,
                                                           long long *__restrict__ first_hit, int32_t *__restrict__ first_ref) {
  const size_t e = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e == 0) cover[n_elems] = 0;
  if (e >= n_elems) return;
  const uint32_t r = ovl_row_of(byte_off, 0, static_cast<uint32_t>(n_rows - 1), e * elem_bytes);
  const size_t s = byte_off[r] / elem_bytes;
  const size_t from = e + 1 >= s + k ? e + 1 - k : s;
  const uint32_t cov = H[e + 1] != H[from] ? 1u : 0u;
  cover[e] = cov;
  if (mask) mask[e] = static_cast<uint8_t>(cov);
  if (hit[e] && H[e] == H[s]) {
    first_hit[r] = static_cast<long long>(e - s);
    const uint32_t t = ent_at[e];
    if (wp_checked(t < m && n_ref != 0, kSiteOverlap)) {
      first_ref[r] = static_cast<int32_t>(ovl_row_of(ref_byte_off, 0, static_cast<uint32_t>(n_ref - 1), static_cast<size_t>(ent_pos[t]) * elem_bytes));
    }
  }
}

// Row i (H, C: the exclusive scans of hit and cover): hits and covered as differences at its ends, keep[i] = 1 where
// hits[i] <= max_hits; keep[n_rows] = 0 closes the flags.  Counted: the rows with a hit.
__global__ __launch_bounds__(kBlock) void ovl_row_results_kernel(const uint32_t *__restrict__ H, const uint32_t *__restrict__ Cv,
                                                                 const uint32_t *__restrict__ byte_off, size_t n_rows, uint32_t elem_bytes,
                                                                 uint32_t max_hits, long long *__restrict__ hits, long long *__restrict__ covered,
                                                                 uint32_t *__restrict__ keep, unsigned long long *__restrict__ counters) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  uint32_t with = 0;
  if (i < n_rows) {
    const size_t a = byte_off[i] / elem_bytes, b = byte_off[i + 1] / elem_bytes;
    const uint32_t h = H[b] - H[a];
    hits[i] = h;
    covered[i] = Cv[b] - Cv[a];
    keep[i] = h <= max_hits ? 1u : 0u;
    with = h != 0 ? 1u : 0u;
  } else if (i == n_rows) {
    keep[i] = 0;
  }
  with = wave_reduce_sum(with);
  if (lane_id() == 0 && with != 0) atomicAdd(counters + kOvlHitRows, static_cast<unsigned long long>(with));
}

// Sorted position s of the reference windows: ref_hit[its flat position] = the mark of its entry (ref_hit starts as zeros)
__global__ __launch_bounds__(kBlock) void ovl_ref_mark_kernel(const uint32_t *__restrict__ val, const uint32_t *__restrict__ ent_of,
                                                              const uint32_t *__restrict__ ent_hit, size_t m, size_t n_ref_elems,
                                                              uint32_t *__restrict__ ref_hit) {
  const size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (s >= m) return;
  const uint32_t t = ent_of[s], p = val[s];
  if (wp_checked(t < m && p < n_ref_elems, kSiteOverlap)) ref_hit[p] = ent_hit[t];
}

// Reference row j (R: the exclusive scan of ref_hit over n_ref_elems + 1 entries): its windows that some corpus window equals
__global__ __launch_bounds__(kBlock) void ovl_ref_rows_kernel(const uint32_t *__restrict__ R, const uint32_t *__restrict__ ref_byte_off, size_t n_ref,
                                                              uint32_t elem_bytes, long long *__restrict__ ref_hits) {
  const size_t j = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j >= n_ref) return;
  ref_hits[j] = R[ref_byte_off[j + 1] / elem_bytes] - R[ref_byte_off[j] / elem_bytes];
}

// Row i that is kept (keep_pos: the exclusive scan of keep): its slot in `kept` and its length in bytes;
// out_len[n_kept] = 0 closes the lengths.
__global__ __launch_bounds__(kBlock) void ovl_kept_kernel(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ keep_pos,
                                                          const uint32_t *__restrict__ byte_off, size_t n_rows, size_t n_kept,
                                                          int32_t *__restrict__ kept, uint32_t *__restrict__ out_len) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i == 0) out_len[n_kept] = 0;
  if (i >= n_rows || !keep[i]) return;
  const uint32_t j = keep_pos[i];
  if (!wp_checked(j < n_kept, kSiteOverlap)) return;
  kept[j] = static_cast<int32_t>(i);
  out_len[j] = byte_off[i + 1] - byte_off[i];
}

}  // namespace wp
