// mask.h — the masked-language-model transform of a batch of model inputs (wp_mlm_mask) and the word index of every
// cell (wp_word_ids); the contract is the section "masking" of include/wordpiece_amd.h.
//
// One kernel, row-major like pack_rows_kernel / inputs_pack_kernel: `lanes` lanes (a power of two, 4..64) share a row,
// a workgroup holds kBlock / lanes rows, and the columns of a row are taken in trips of `lanes`.  What a cell needs of
// its neighbours — was the column before it outside or a word of its own, where does its word start, how many words
// began since the last special — the lanes of a row exchange through three wave64 ballots per trip, each masked to the
// row's lane group, and three values carried in registers from trip to trip.  EVERY lane of a workgroup runs every trip:
// lanes of rows behind n_rows and of columns behind max_len vote "outside", load nothing and store nothing.
//
// A cell is one 4-byte coalesced load, one byte of the per-id class table (an L2-resident gather) and up to three
// 4-byte coalesced stores; the random draws are integer arithmetic in registers.
#pragma once
#include "primitives.h"  // bits_up_to, top_bit

namespace wp {

struct MaskGeom {
  int max_len;
  int32_t cls_id, sep_id, pad_id, mask_id, ignore_id;
  int whole_word;
  long long vocab_size;
  unsigned long long select_q32, mask_q32, random_q32, seed, row_base;
};

// the counters of a call, 64 bits each, in this order behind d_scalars + kScalarMask
enum MaskCounter { kMaskWords = 0, kMaskSelected, kMaskUnits, kMaskMasked, kMaskRandom, kMaskKept, kMaskCounters };

__host__ __device__ inline unsigned long long mask_mix(unsigned long long x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}
// the row's half of the draw: mix(seed + G * (row + 1))
__host__ __device__ inline unsigned long long mask_row_key(unsigned long long seed, unsigned long long row) {
  return mask_mix(seed + 0x9E3779B97F4A7C15ull * (row + 1ull));
}
// draw(seed, row, col, stream), a 32-bit value
__host__ __device__ inline unsigned long long mask_draw(unsigned long long row_key, unsigned long long col, unsigned stream) {
  return mask_mix(row_key + 0x9E3779B97F4A7C15ull * (4ull * col + stream + 1ull)) >> 32;
}

// The largest grid of a call: 8 workgroups for each of the 256 CUs.  Every workgroup ends with its atomics on the SAME
// six counters.  With one workgroup per row block (377,125 at 1.5 M rows of 128) the call cost 4.6 ms whether it moved
// 8, 12 or 16 B per cell (profiles/mask_probe.jsonl, line 1): not the bytes — the reading that
// fits is those atomics, serialised.  A capped grid bounds them by the machine, not by the batch.
constexpr unsigned kMaskMaxGrid = 2048;

// MASK: `out` and `labels` are written; WORD_IDS: `word_ids` is.  `in` and `out` may be the same buffer: a lane reads
// its own cell only, before it stores there.  tok_class[x] = wp_vocab_token_flags(x) for 0 <= x < g.vocab_size.
// n_blocks = ceil(n_rows / (kBlock / lanes)) row blocks are dealt to the workgroups of the grid round robin (at most
// kMaskMaxGrid of them).  counters: kMaskCounters 64-bit sums, at most one global atomic per counter and workgroup.
template <bool MASK, bool WORD_IDS>
__global__ __launch_bounds__(kBlock) void mask_kernel(const int32_t *in, const int32_t *__restrict__ lengths, size_t n_rows, size_t n_blocks,
                                                      MaskGeom g, int lanes, const uint8_t *__restrict__ tok_class, int32_t *out,
                                                      int32_t *__restrict__ labels, int32_t *__restrict__ word_ids,
                                                      unsigned long long *__restrict__ counters) {
  __shared__ unsigned long long s_cnt[kMaskCounters];
  if (threadIdx.x < kMaskCounters) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int rows_per_block = kBlock / lanes;
  const int l = threadIdx.x % lanes;                       // the lane's place in its row's group
  const int shift = (threadIdx.x & (kWave - 1)) - l;       // the group's first lane in the wave
  const unsigned long long group = bits_up_to(lanes - 1);  // (after the shift)
  const unsigned long long le = bits_up_to(l);
  unsigned long long n_words = 0, n_sel = 0, n_units = 0, n_masked = 0, n_random = 0, n_kept = 0;
  // a workgroup takes the row blocks blockIdx.x, blockIdx.x + gridDim.x, ... (uniform: all its lanes run every trip of
  // every block), so that the counters cost one set of global atomics per RESIDENT workgroup, not per row block
  for (size_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const size_t r = blk * rows_per_block + threadIdx.x / lanes;
    const bool live = r < n_rows;
    int len = 0;
    if (live) {
      len = g.max_len;
      if (lengths) len = max(0, min(lengths[r], g.max_len));
    }
    const size_t base = live ? r * static_cast<size_t>(g.max_len) : 0;
    const unsigned long long row_key = mask_row_key(g.seed, g.row_base + r);
    // carried from trip to trip, the same in every lane of the group
    int open_start = 0;      // the column the open word starts in
    int count = 0;           // words begun since the last outside column
    bool prev_breaks = true;  // column c - 1 was outside or a word of its own (or c == 0)
    // (uniform: every lane of the workgroup runs every trip; counted in 64 bits: max_len may be close to INT32_MAX)
    for (long long trip0 = 0; trip0 < g.max_len; trip0 += lanes) {
      const bool cell = live && trip0 + l < g.max_len;
      const int col0 = static_cast<int>(trip0), col = cell ? col0 + l : 0;  // (col is used for cells only)
      int32_t x = 0;
      if (cell) x = in[base + col];
      bool outside = !cell || col >= len || x < 0 || x >= g.vocab_size || (g.cls_id >= 0 && x == g.cls_id) ||
                     (g.sep_id >= 0 && x == g.sep_id) || (g.pad_id >= 0 && x == g.pad_id);
      // (the contract's own range test above is what guards the lookup — an id outside the vocabulary is valid input,
      // not a violation — so kSiteMask counts only if that test and this one ever disagree)
      uint32_t f = 0;
      if (!outside) {
        const bool ok = static_cast<unsigned long long>(x) < static_cast<unsigned long long>(g.vocab_size);
        if (wp_in_bounds(ok, kSiteMask) && ok) {
          f = tok_class[x];
        } else {
          outside = true;
        }
      }
      const bool solo = !outside && (f & 6u) != 0;
      const bool cont = !outside && !solo && (f & 1u) == 0;
      const unsigned long long out_bits = (__ballot(outside) >> shift) & group;
      const unsigned long long brk_bits = (__ballot(outside || solo) >> shift) & group;
      const bool before = l == 0 ? prev_breaks : ((brk_bits >> (l - 1)) & 1ull) != 0;
      const bool start = !outside && (!cont || before);
      const unsigned long long start_bits = (__ballot(start) >> shift) & group;
      // w(c): the highest start bit at or below the lane, else the word that was open when the trip began
      const unsigned long long s_le = start_bits & le;
      const int w = s_le ? col0 + top_bit(s_le) : open_start;
      // the words begun behind the last outside column at or below the lane
      const unsigned long long o_le = out_bits & le;
      const int words = o_le ? __popcll(s_le & ~bits_up_to(top_bit(o_le))) : count + __popcll(s_le);
      if (cell) {
        if (WORD_IDS) word_ids[base + col] = outside ? -1 : words - 1;
        if (start) n_words++;
        if (MASK) {
          int32_t y = x, label = g.ignore_id;
          // (a unit is selectable when its first cell is no word of its own; a cell's word is solo exactly when the cell is)
          if (!outside && !solo) {
            const int unit = g.whole_word ? w : col;
            if (mask_draw(row_key, static_cast<unsigned long long>(unit), 0u) < g.select_q32) {
              label = x;
              n_sel++;
              if (unit == col) n_units++;
              const unsigned long long t = mask_draw(row_key, static_cast<unsigned long long>(col), 1u);
              if (t < g.mask_q32) {
                y = g.mask_id;
                n_masked++;
              } else if (t < g.mask_q32 + g.random_q32) {
                y = static_cast<int32_t>((mask_draw(row_key, static_cast<unsigned long long>(col), 2u) *
                                          static_cast<unsigned long long>(g.vocab_size)) >> 32);
                n_random++;
              } else {
                n_kept++;
              }
            }
          }
          out[base + col] = y;
          labels[base + col] = label;
        }
      }
      // the carries, from the whole group's bits
      if (start_bits) open_start = col0 + top_bit(start_bits);
      count = out_bits ? __popcll(start_bits & ~bits_up_to(top_bit(out_bits))) : count + __popcll(start_bits);
      prev_breaks = ((brk_bits >> (lanes - 1)) & 1ull) != 0;
    }
  }
  // a wave sums its lanes' counts first: 4 LDS atomics per counter and workgroup (every lane is here: the loops are uniform)
  unsigned long long sums[kMaskCounters] = {n_words, n_sel, n_units, n_masked, n_random, n_kept};
#pragma unroll
  for (int k = 0; k < (MASK ? kMaskCounters : 1); k++) {
    unsigned long long v = sums[k];
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && v != 0) atomicAdd(&s_cnt[k], v);
  }
  __syncthreads();
  if (threadIdx.x < kMaskCounters && s_cnt[threadIdx.x] != 0) atomicAdd(&counters[threadIdx.x], s_cnt[threadIdx.x]);
}

}  // namespace wp
