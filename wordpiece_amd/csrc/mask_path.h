// mask_path.h — masking on a context (include/wordpiece_amd.h, section "masking"; kernel: mask.h): the argument rules,
// the one launch over device buffers, and the buffers of a host call.
#pragma once
#include "context.h"
#include "mask.h"
#include "rows.h"  // lanes_for

namespace wp {

constexpr unsigned long long kQ32One = 1ull << 32;

// wp_vocab_token_flags, and the class byte of an id on the device (mask.h)
static int32_t token_flags(const HostToken &t) { return (t.is_prefix ? 1 : 0) | (t.is_special ? 2 : 0) | (t.is_malformed ? 4 : 0); }

// every argument rule of a mask (mask_call) or word-ids call that needs no device
static MaskGeom check_mask_spec(const wp_vocab *v, const wp_mask_spec *spec, size_t n_rows, bool mask_call) {
  if (!spec) throw std::invalid_argument("mask: spec is NULL");
  if (spec->max_len < 1) throw std::invalid_argument("mask: max_len must be at least 1");
  MaskGeom g{};
  g.max_len = spec->max_len;
  g.cls_id = spec->cls_id;
  g.sep_id = spec->sep_id;
  g.pad_id = spec->pad_id;
  g.vocab_size = static_cast<long long>(v->hv.tokens.size());
  if (mask_call) {
    if (spec->whole_word != 0 && spec->whole_word != 1) throw std::invalid_argument("mask: whole_word must be 0 or 1");
    if (spec->select_q32 > kQ32One) throw std::invalid_argument("mask: select_q32 must be at most 2^32");
    if (spec->mask_q32 > kQ32One) throw std::invalid_argument("mask: mask_q32 must be at most 2^32");
    if (spec->random_q32 > kQ32One) throw std::invalid_argument("mask: random_q32 must be at most 2^32");
    if (spec->mask_q32 + spec->random_q32 > kQ32One) throw std::invalid_argument("mask: mask_q32 + random_q32 must be at most 2^32");
    if (spec->mask_id < 0) throw std::invalid_argument("mask: mask_id must be at least 0");
    g.mask_id = spec->mask_id;
    g.ignore_id = spec->ignore_id;
    g.whole_word = spec->whole_word;
    g.select_q32 = spec->select_q32;
    g.mask_q32 = spec->mask_q32;
    g.random_q32 = spec->random_q32;
    g.seed = spec->seed;
    g.row_base = spec->row_base;
  }
  if (n_rows > static_cast<size_t>(INT32_MAX)) throw std::length_error("mask: more rows than INT32_MAX");
  if (n_rows > SIZE_MAX / sizeof(int32_t) / static_cast<size_t>(spec->max_len)) {
    throw std::length_error("mask: n_rows * max_len is too large");
  }
  return g;
}

// the statistics of a mask or word-ids call before its counters are known (all there is to say of a call without rows)
static wp_mask_stats &begin_mask_stats(wp_vocab *v, size_t n_rows, int whole_word) {
  v->stats.mask_call = 1;
  v->stats.mask = wp_mask_stats{};
  v->stats.mask.n_rows = static_cast<int64_t>(n_rows);
  v->stats.mask.whole_word = whole_word;
  return v->stats.mask;
}

// One launch of mask_kernel over device buffers on c's stream, one wait (for the counters), the statistics of the call.
// d_masked == nullptr: the word-ids form.
static void mask_on_device(wp_vocab *v, Context *c, const int32_t *d_in, const int32_t *d_lengths, size_t n_rows, const MaskGeom &g,
                           int32_t *d_masked, int32_t *d_labels, int32_t *d_word_ids) {
  const bool mask_call = d_masked != nullptr;
  wp_mask_stats &ms = begin_mask_stats(v, n_rows, mask_call ? g.whole_word : 0);
  if (n_rows == 0) return;
  hipStream_t st = c->stream;
  if (!c->d_tok_class) {  // one byte per id: wp_vocab_token_flags
    std::vector<uint8_t> cls(v->hv.tokens.size());
    for (size_t i = 0; i < cls.size(); i++) cls[i] = static_cast<uint8_t>(token_flags(v->hv.tokens[i]));
    c->d_tok_class = upload(cls, st);
    WP_HIP(hipStreamSynchronize(st));  // cls is a local
  }
  static_assert(scalar_end(kScalarMask) - kScalarMask == 2 * kMaskCounters, "the slot kScalarMask holds the counters of a mask call");
  unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarMask);
  clear_scalars(c, kScalarMask, kScalarMask, st);
  const int lanes = lanes_for(g.max_len);
  const size_t n_blocks = (n_rows + static_cast<size_t>(kBlock / lanes) - 1) / static_cast<size_t>(kBlock / lanes);
  const dim3 grid(static_cast<unsigned>(std::min<size_t>(n_blocks, kMaskMaxGrid))), block(kBlock);
  if (!mask_call) {
    hipLaunchKernelGGL((mask_kernel<false, true>), grid, block, 0, st, d_in, d_lengths, n_rows, n_blocks, g, lanes,
                       c->d_tok_class, d_masked, d_labels,
                       d_word_ids, d_cnt);
  } else if (d_word_ids) {
    hipLaunchKernelGGL((mask_kernel<true, true>), grid, block, 0, st, d_in, d_lengths, n_rows, n_blocks, g, lanes,
                       c->d_tok_class, d_masked, d_labels,
                       d_word_ids, d_cnt);
  } else {
    hipLaunchKernelGGL((mask_kernel<true, false>), grid, block, 0, st, d_in, d_lengths, n_rows, n_blocks, g, lanes,
                       c->d_tok_class, d_masked, d_labels,
                       d_word_ids, d_cnt);
  }
  WP_LAUNCH_CHECK();
  queue_scalar_slots(c, kScalarMask, kScalarMask, st);
  WP_HIP(hipStreamSynchronize(st));
  throw_if_oob(kSiteMask, "masking", "class lookups outside the vocabulary skipped");
  const unsigned long long *h_cnt = reinterpret_cast<const unsigned long long *>(c->h_scalars + kScalarMask);
  ms.n_words = static_cast<int64_t>(h_cnt[kMaskWords]);
  ms.n_selected = static_cast<int64_t>(h_cnt[kMaskSelected]);
  ms.n_selected_units = static_cast<int64_t>(h_cnt[kMaskUnits]);
  ms.n_masked = static_cast<int64_t>(h_cnt[kMaskMasked]);
  ms.n_random = static_cast<int64_t>(h_cnt[kMaskRandom]);
  ms.n_kept = static_cast<int64_t>(h_cnt[kMaskKept]);
}

// The host form as far as the device: ids (and lengths) go up into c->pad_buf, one launch, and the 1..3 blocks of n_rows *
// max_len int32 the caller asked for lie there until the handle's next call: ids | masked, labels | word_ids | lengths.
struct MaskBatch {
  int32_t *d_masked = nullptr, *d_labels = nullptr, *d_word_ids = nullptr;
};
static MaskBatch mask_from_host(wp_vocab *v, Context *c, const int32_t *input_ids, const int32_t *lengths, size_t n_rows, const MaskGeom &g,
                                bool mask_call, bool want_word_ids) {
  const size_t cells = n_rows * static_cast<size_t>(g.max_len);
  Arena a(&c->pad_buf);
  MaskBatch b;
  int32_t *d_in = nullptr, *d_len = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_in = a.take<int32_t>(cells);
    if (mask_call) {
      b.d_masked = a.take<int32_t>(cells);
      b.d_labels = a.take<int32_t>(cells);
    }
    if (want_word_ids) b.d_word_ids = a.take<int32_t>(cells);
    // + 4: the 16 bytes this block always ended with; mask_kernel loads and stores nothing behind n_rows
    d_len = a.take<int32_t>(n_rows + 4);
    if (pass == 0) a.commit();
  }
  WP_HIP(hipMemcpyAsync(d_in, input_ids, cells * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  if (lengths) WP_HIP(hipMemcpyAsync(d_len, lengths, n_rows * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  mask_on_device(v, c, d_in, lengths ? d_len : nullptr, n_rows, g, b.d_masked, b.d_labels, b.d_word_ids);
  return b;
}

}  // namespace wp
