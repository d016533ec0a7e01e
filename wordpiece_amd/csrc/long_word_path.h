// long_word_path.h — the host half of the long-word path (walk.h, "long words"), which the Linear and the fast encoder
// share: their kernels differ only in how a position finds its next one (*_next_kernel) and in how ids leave (*_emit_kernel).
#pragma once
#include "context.h"
#include "walk.h"

namespace wp {

struct LongWordList {
  uint32_t nw = 0, total = 0, longest = 0;  // words (0: none, nothing was queued), their positions, the longest word
  std::vector<uint32_t> h_off;              // first position of every word in the concatenation, and the total
  dim3 grid() const { return dim3(cdiv(total, kBlock)); }
};

// The list the collect kernel left: downloaded, its lengths turned into offsets, those uploaded, the fail flags cleared.
// h_off is the source of that upload: the caller synchronises behind the launch of its *_next_kernel (which it has to
// queue anyway before the host has anything else to do) and only then lets go of the list.
static LongWordList long_word_offsets(Context *c, const LongWord *d_lw, uint32_t lw_cap, uint32_t *d_lw_off, uint32_t *d_lw_fail,
                                      hipStream_t st) {
  LongWordList l;
  fetch_scalars(c, kScalarLongWords);
  l.nw = std::min(c->h_scalars[kScalarLongWords], lw_cap);
  if (l.nw == 0) return l;
  std::vector<LongWord> h_lw(l.nw);
  WP_HIP(hipMemcpyAsync(h_lw.data(), d_lw, sizeof(LongWord) * l.nw, hipMemcpyDeviceToHost, st));
  WP_HIP(hipStreamSynchronize(st));
  l.h_off.resize(l.nw + 1);
  uint64_t total64 = 0;
  for (uint32_t i = 0; i < l.nw; i++) {
    l.h_off[i] = static_cast<uint32_t>(total64);
    total64 += h_lw[i].end - h_lw[i].begin;
    l.longest = std::max(l.longest, h_lw[i].end - h_lw[i].begin);
  }
  l.h_off[l.nw] = static_cast<uint32_t>(total64);
  l.total = static_cast<uint32_t>(total64);  // <= n_text < 2^31
  WP_HIP(hipMemcpyAsync(d_lw_off, l.h_off.data(), sizeof(uint32_t) * (l.nw + 1), hipMemcpyHostToDevice, st));
  WP_HIP(hipMemsetAsync(d_lw_fail, 0, sizeof(uint32_t) * l.nw, st));
  return l;
}

// Behind the *_next_kernel: the positions on the chain of every word by pointer doubling (jump_a: every position's next
// one; jump_b: scratch), and the words whose chain ends in no token
static void long_word_chains(const LongWordList &l, uint32_t *jump_a, uint32_t *jump_b, const int32_t *d_lid, uint8_t *d_mark,
                             const uint32_t *d_lw_off, uint32_t *d_lw_fail, hipStream_t st) {
  for (uint32_t reach = 1; reach < l.longest; reach *= 2) {  // after r rounds: chain prefixes of length 2^r
    hipLaunchKernelGGL(long_word_mark_kernel, l.grid(), dim3(kBlock), 0, st, jump_a, l.total, d_mark);
    hipLaunchKernelGGL(long_word_double_kernel, l.grid(), dim3(kBlock), 0, st, jump_a, l.total, jump_b);
    std::swap(jump_a, jump_b);
  }
  hipLaunchKernelGGL(long_word_mark_kernel, l.grid(), dim3(kBlock), 0, st, jump_a, l.total, d_mark);
  hipLaunchKernelGGL(long_word_fail_kernel, l.grid(), dim3(kBlock), 0, st, d_lid, d_mark, d_lw_off, l.nw, l.total, d_lw_fail);
}

}  // namespace wp
