// count_path.h — word counts on a context (include/wordpiece_amd.h, section "word counts"; kernels: count.h): the
// argument rules, the launches over a device text, the rounds of the grouping and the buffers of a call.
#pragma once
#include "context.h"
#include "count.h"
#include "group_path.h"
#include "normalize.h"

namespace wp {

// the spec of a call with its defaults filled in
struct CountPlan {
  int order = 0, terminator = -1, hash_bits = 64;
  uint32_t max_bytes = 256;
  bool want_index = false;
  unsigned long long min_count = 1;
};

// every rule of the spec, each with the field it is about; nothing here needs a device
static CountPlan check_count_spec(const wp_count_spec *spec, const wp_word_counts *out) {
  if (!spec) throw std::invalid_argument("count: spec is NULL");
  if (!out) throw std::invalid_argument("count: out is NULL");
  if (spec->order != WP_COUNT_ORDER_FIRST && spec->order != WP_COUNT_ORDER_COUNT) throw std::invalid_argument("count: order must be 0 or 1");
  if (spec->max_word_bytes < 0 || spec->max_word_bytes > kCountMaxWordBytes) {
    throw std::invalid_argument("count: max_word_bytes must be 0 (256) or in [1, 1024]");
  }
  if (spec->terminator < -1 || spec->terminator > 255) throw std::invalid_argument("count: terminator must be in [-1, 255]");
  check_want("count", spec->want, WP_COUNT_WANT_INDEX);
  const int hash_bits = checked_hash_bits("count", spec->hash_bits);
  if (spec->reserved != 0) throw std::invalid_argument("count: reserved must be 0");
  if (spec->min_count < 0) throw std::invalid_argument("count: min_count must not be negative");
  CountPlan p;
  p.order = spec->order;
  p.terminator = spec->terminator;
  p.hash_bits = hash_bits;
  p.max_bytes = spec->max_word_bytes == 0 ? 256u : static_cast<uint32_t>(spec->max_word_bytes);
  p.want_index = (spec->want & WP_COUNT_WANT_INDEX) != 0;
  p.min_count = spec->min_count == 0 ? 1ull : static_cast<unsigned long long>(spec->min_count);
  return p;
}

// the statistics of a count call before anything is known of its text
static wp_count_stats &begin_count_stats(wp_vocab *v) {
  v->stats.count_call = 1;
  v->stats.count = wp_count_stats{};
  return v->stats.count;
}

// the table of an empty text: no word, one offset; no device needed
static wp_word_counts count_of_nothing(wp_vocab *v) {
  begin_count_stats(v);
  wp_word_counts h{};
  h.word_off = static_cast<int64_t *>(zeroed(sizeof(int64_t)));
  return h;
}

// The table of the text at d_text (buffer contract of the device encode), on c's stream.  The results are device
// pointers into c->count_out (R->words, word_off, counts, word_index), valid until the handle's next call; the counted
// text itself is in c->norm_buf.  Waits: the pre-pass's own, the word count, the listed count, one per round, the kept count.
static void count_on_device(wp_vocab *v, Context *c, const uint8_t *d_text, size_t nbytes, const CountPlan &plan, wp_word_counts *R) {
  wp_count_stats &cs = begin_count_stats(v);
  *R = wp_word_counts{};
  hipStream_t st = c->stream;
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  const int term = plan.terminator >= 0 ? 1 : 0;
  NormResult norm;
  // WP_OPT_STAGE_TIMING: the marks of a count call are kMarkStart (behind the pre-pass), kMarkCounted (the words are listed),
  // kMarkSorted (the rounds are over) and kMarkWalked (the table is written)
  const bool timing = v->stage_timing && nbytes != 0;
  if (nbytes != 0) normalize_on_device(c, d_text, nbytes, v->normalize, false, timing, norm);  // (flags 0: the valid UTF-8 of the text)
  RadixStats *rs = begin_stage_timing(c, timing, st);
  const size_t nb = norm.nbytes;  // (at most UINT32_MAX: the pre-pass throws std::length_error beyond)
  cs.n_text_bytes = static_cast<int64_t>(nb);
  const uint8_t *text = norm.text;

  // ---- word starts and ends ---------------------------------------------------------------------------------------
  size_t n_words = 0;
  const unsigned tiles = cdiv(nb + 1, kCountTile);
  Arena aux(&c->count_aux, guard);
  uint32_t *d_ts = nullptr, *d_te = nullptr, *d_tmp0 = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_ts = aux.take<uint32_t>(static_cast<size_t>(tiles) + 1);
    d_te = aux.take<uint32_t>(static_cast<size_t>(tiles) + 1);
    d_tmp0 = aux.take<uint32_t>(cdiv(tiles, kScanTile) + 8);
    if (pass == 0) aux.commit();
  }
  aux.arm(st);
  if (nb != 0) {
    clear_scalars(c, kScalarCountWords, kScalarCount, st);
    hipLaunchKernelGGL(count_starts_kernel<false>, dim3(tiles), dim3(kBlock), 0, st, text, nb, c->d_cls_bmp, d_ts, d_te,
                       static_cast<uint32_t *>(nullptr), static_cast<uint32_t *>(nullptr), size_t(0));
    device_exclusive_scan(d_ts, d_ts, tiles, d_tmp0, nullptr, st, nullptr, reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarCountWords));
    device_exclusive_scan(d_te, d_te, tiles, d_tmp0, nullptr, st);
    WP_LAUNCH_CHECK();
    queue_scalar_slots(c, kScalarCountWords, kScalarCountWords, st);
    WP_HIP(hipStreamSynchronize(st));
    unsigned long long words64;
    std::memcpy(&words64, c->h_scalars + kScalarCountWords, sizeof(words64));
    if (words64 >= (1ull << 31)) throw std::length_error("count: the text has 2^31 words or more");
    n_words = static_cast<size_t>(words64);
  }
  cs.n_words = static_cast<int64_t>(n_words);
  R->n_words = cs.n_words;

  // ---- the per-word arrays ------------------------------------------------------------------------------------------
  const size_t n1 = n_words + 1;
  const size_t tmp_words = radix_tmp_words<uint64_t>(n_words);
  Arena wa(&c->count_words, guard);
  uint32_t *d_start = nullptr, *d_end = nullptr, *d_items0 = nullptr, *d_items1 = nullptr, *d_head = nullptr, *d_run = nullptr, *d_head_pos = nullptr,
           *d_agree = nullptr, *d_agree_pos = nullptr, *d_left = nullptr, *d_left_pos = nullptr, *d_v0 = nullptr, *d_v1 = nullptr,
           *d_gfirst = nullptr, *d_gcount = nullptr, *d_rtmp = nullptr, *d_stmp = nullptr;
  int32_t *d_wgroup = nullptr, *d_gfinal = nullptr;
  uint64_t *d_k0 = nullptr, *d_k1 = nullptr;
  if (n_words != 0) {
    for (int pass = 0; pass < 2; pass++) {
      d_start = wa.take<uint32_t>(n_words);
      d_end = wa.take<uint32_t>(n_words);
      d_wgroup = wa.take<int32_t>(n_words);
      d_items0 = wa.take<uint32_t>(n_words);
      d_items1 = wa.take<uint32_t>(n_words);
      d_head = wa.take<uint32_t>(n1);
      d_run = wa.take<uint32_t>(n1);
      d_head_pos = wa.take<uint32_t>(n1);
      d_agree = wa.take<uint32_t>(n1);
      d_agree_pos = wa.take<uint32_t>(n1);
      d_left = wa.take<uint32_t>(n1);
      d_left_pos = wa.take<uint32_t>(n1);
      d_k0 = wa.take<uint64_t>(n_words);
      d_k1 = wa.take<uint64_t>(n_words);
      d_v0 = wa.take<uint32_t>(n_words);
      d_v1 = wa.take<uint32_t>(n_words);
      d_gfirst = wa.take<uint32_t>(n_words);
      d_gcount = wa.take<uint32_t>(n_words);
      d_gfinal = wa.take<int32_t>(n_words);
      d_rtmp = wa.take<uint32_t>(tmp_words);
      d_stmp = wa.take<uint32_t>(cdiv(n1, kScanTile) + 8);
      if (pass == 0) wa.commit();
    }
    wa.arm(st);
    hipLaunchKernelGGL(count_starts_kernel<true>, dim3(tiles), dim3(kBlock), 0, st, text, nb, c->d_cls_bmp, d_ts, d_te, d_start, d_end, n_words);
    // the listed words (not long), in text order: the items of round 0
    hipLaunchKernelGGL(count_listed_kernel, count_grid(n_words), dim3(kBlock), 0, st, d_start, d_end, n_words, plan.max_bytes, d_head, d_wgroup);
    device_exclusive_scan(d_head, d_run, n_words, d_stmp, c->d_scalars + kScalarCountListed, st);
    compact_flagged(d_head, d_run, n_words, nullptr, d_items0, st);
    WP_LAUNCH_CHECK();
    if (timing) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));
    queue_scalar_slots(c, kScalarCountListed, kScalarCountListed, st);
    WP_HIP(hipStreamSynchronize(st));
  }
  if (timing && n_words == 0) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));
  size_t m = n_words != 0 ? c->h_scalars[kScalarCountListed] : 0;
  cs.n_long = static_cast<int64_t>(n_words - m);

  // ---- the rounds: hash, sort, compare with the head of the run, leftovers on ------------------------------------------
  const uint64_t mask = plan.hash_bits >= 64 ? ~0ull : (1ull << plan.hash_bits) - 1ull;
  size_t n_groups = 0;
  uint32_t *items = d_items0, *next = d_items1;
  while (m != 0) {
    hipLaunchKernelGGL(count_keys_kernel, count_grid(m), dim3(kBlock), 0, st, text, d_start, d_end, items, m, static_cast<uint64_t>(cs.n_rounds), mask,
                       plan.max_bytes, d_k0);
    const int cur = radix_sort_pairs<uint64_t>(d_k0, d_v0, d_k1, d_v1, m, 0, plan.hash_bits, d_rtmp, tmp_words, st, rs, true);
    const uint64_t *keys = cur ? d_k1 : d_k0;
    const uint32_t *vals = cur ? d_v1 : d_v0;
    uint32_t *d_runs = c->d_scalars + kScalarCountRuns;
    group_runs(keys, m, d_head, d_run, d_head_pos, d_stmp, d_runs, st);
    hipLaunchKernelGGL(count_verify_kernel, count_grid(m), dim3(kBlock), 0, st, text, d_start, d_end, items, vals, d_head, d_run, d_head_pos, m, n_words,
                       plan.max_bytes, static_cast<uint32_t>(n_groups), d_agree, d_left, d_wgroup);
    device_exclusive_scan(d_agree, d_agree_pos, m + 1, d_stmp, nullptr, st);
    hipLaunchKernelGGL(count_groups_kernel, count_grid(m), dim3(kBlock), 0, st, items, vals, d_head_pos, d_agree_pos, d_runs, m, d_gfirst + n_groups,
                       d_gcount + n_groups);
    carry_leftovers(d_left, d_left_pos, m, items, next, d_stmp, c->d_scalars + kScalarCountLeft, st);
    n_groups += end_round(c, kScalarCountRuns, kScalarCountLeft, "count", "word", &m, &cs, st);
    std::swap(items, next);
  }

  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));

  // ---- filter, order, gather ------------------------------------------------------------------------------------------
  size_t n_kept = 0;
  unsigned long long kept_bytes = 0;
  if (n_groups != 0) {
    hipLaunchKernelGGL(count_filter_kernel, count_grid(n_groups), dim3(kBlock), 0, st, d_gfirst, d_gcount, n_groups, plan.min_count, d_start, d_end,
                       d_head, reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarCount) + kCountKeptBytes);
    device_exclusive_scan(d_head, d_run, n_groups, d_stmp, c->d_scalars + kScalarCountKept, st);
    WP_HIP(hipMemsetAsync(d_gfinal, 0xff, n_groups * sizeof(int32_t), st));
    WP_LAUNCH_CHECK();
    queue_scalar_slots(c, kScalarCountKept, kScalarCount, st);
    WP_HIP(hipStreamSynchronize(st));
    n_kept = c->h_scalars[kScalarCountKept];
    std::memcpy(&kept_bytes, c->h_scalars + kScalarCount, sizeof(kept_bytes));
  }
  cs.n_distinct = static_cast<int64_t>(n_kept);
  cs.n_below_min = static_cast<int64_t>(n_groups - n_kept);
  const size_t pool_bytes = static_cast<size_t>(kept_bytes) + n_kept * static_cast<size_t>(term);
  const bool index = plan.want_index && n_words != 0;
  Arena oa(&c->count_out, guard);
  uint8_t *d_pool = nullptr;
  long long *d_word_off = nullptr, *d_counts = nullptr;
  int32_t *d_index = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_pool = oa.take<uint8_t>(pool_bytes);
    d_word_off = oa.take<long long>(n_kept + 1);
    d_counts = oa.take<long long>(n_kept);
    if (index) d_index = oa.take<int32_t>(n_words);
    if (pass == 0) oa.commit();
  }
  oa.arm(st);
  if (n_kept != 0) {
    uint32_t *d_kept_group = d_items0, *d_len = d_agree, *d_len_pos = d_agree_pos, *d_src = d_left;  // (the rounds are over)
    hipLaunchKernelGGL(count_order_keys_kernel, count_grid(n_groups), dim3(kBlock), 0, st, d_head, d_run, d_gfirst, d_gcount, n_groups, n_kept,
                       plan.order == WP_COUNT_ORDER_COUNT ? 1 : 0, d_k0, d_kept_group);
    const int bits = plan.order == WP_COUNT_ORDER_COUNT ? 64 : std::max(1, bit_length(n_words));
    const int cur = radix_sort_pairs<uint64_t>(d_k0, d_v0, d_k1, d_v1, n_kept, 0, bits, d_rtmp, tmp_words, st, rs, true);
    hipLaunchKernelGGL(count_emit_kernel, count_grid(n_kept), dim3(kBlock), 0, st, cur ? d_v1 : d_v0, d_kept_group, d_gfirst, d_gcount, d_start, d_end,
                       n_kept, n_groups, d_counts, d_len, d_src, d_gfinal);
    device_exclusive_scan(d_len, d_len_pos, n_kept + 1, d_stmp, nullptr, st);
    hipLaunchKernelGGL(group_offsets_kernel, count_grid(n_kept + 1), dim3(kBlock), 0, st, d_len_pos, n_kept, term, d_word_off);
    hipLaunchKernelGGL(count_gather_kernel, count_grid(pool_bytes), dim3(kBlock), 0, st, text, nb, d_word_off, d_src, n_kept, plan.terminator,
                       pool_bytes, d_pool);
  } else {
    WP_HIP(hipMemsetAsync(d_word_off, 0, sizeof(long long), st));
  }
  if (index) {
    hipLaunchKernelGGL(count_index_kernel, count_grid(n_words), dim3(kBlock), 0, st, d_wgroup, d_gfinal, n_words, n_groups, d_index);
  }
  WP_LAUNCH_CHECK();
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkWalked], st));
  WP_HIP(hipStreamSynchronize(st));
  if (timing) {  // wp_stats, as the header's section says: the stage times of this call in the fields an encode times itself in
    const float words = mark_ms(c, kMarkStart, kMarkCounted), rounds = mark_ms(c, kMarkCounted, kMarkSorted), table = mark_ms(c, kMarkSorted, kMarkWalked);
    v->stats.ms_normalize = norm.ms;
    v->stats.ms_decode = words;
    v->stats.ms_sa = rounds;
    v->stats.ms_walk = table;
    v->stats.ms_total = norm.ms + words + rounds + table;
    end_stage_timing(v, c);
  }
  throw_if_group_oob(kSiteCount, "word counts", "stores or gathers outside the word, group or table arrays skipped");
  check_arena_guard(c, aux, st, "count");
  check_arena_guard(c, wa, st, "count");
  check_arena_guard(c, oa, st, "count");
  R->words = pool_bytes ? d_pool : nullptr;
  R->word_off = reinterpret_cast<int64_t *>(d_word_off);
  R->counts = n_kept ? reinterpret_cast<int64_t *>(d_counts) : nullptr;
  R->word_index = index ? d_index : nullptr;
  R->n_distinct = static_cast<int64_t>(n_kept);
  R->n_bytes = static_cast<int64_t>(pool_bytes);
}

}  // namespace wp
