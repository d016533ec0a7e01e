// learn_path.h — the vocabulary learner on a context (include/wordpiece_amd.h, section "vocabulary learner"; kernels:
// learn.h): the argument rules, the launches over a device table, the rounds of the grouping, the search and the
// buffers of a call.  Launches of one search step: per iteration one split (none in iteration 0), one clear, one sum and
// one level launch per token length that has tokens, so at most num_iterations * (max_token_chars + 3); one wait per step.
#pragma once
#include <array>

#include "context.h"
#include "group_path.h"
#include "learn.h"

namespace wp {

// the spec of a call with its defaults filled in; the reserved tokens back to back with 32-bit offsets
struct LearnPlan {
  long long vocab_size = 0, lower = 0, upper = 0, slack = 0;
  int iterations = 0, max_chars = 0, max_unique = 0, terminator = -1, hash_bits = 64;
  std::vector<uint8_t> res;
  std::vector<uint32_t> res_off;
};

// every rule of the spec, each with the field it is about; nothing here needs a device
static LearnPlan check_learn_spec(const wp_learn_spec *spec, const wp_learned_vocab *out) {
  if (!spec) throw std::invalid_argument("learn: spec is NULL");
  if (!out) throw std::invalid_argument("learn: out is NULL");
  if (spec->vocab_size < 1) throw std::invalid_argument("learn: vocab_size must be at least 1");
  if (spec->max_token_chars < 1 || spec->max_token_chars > kLearnMaxChars) throw std::invalid_argument("learn: max_token_chars must be in [1, 64]");
  if (spec->num_iterations < 1) throw std::invalid_argument("learn: num_iterations must be at least 1");
  if (spec->lower_thresh < 1) throw std::invalid_argument("learn: lower_thresh must be at least 1");
  if (spec->upper_thresh < 1) throw std::invalid_argument("learn: upper_thresh must be at least 1");
  if (spec->lower_thresh > spec->upper_thresh) throw std::invalid_argument("learn: lower_thresh must not be above upper_thresh");
  if (spec->slack < 0) throw std::invalid_argument("learn: slack must not be negative");
  if (spec->max_unique_chars < 0) throw std::invalid_argument("learn: max_unique_chars must not be negative");
  if (spec->terminator < -1 || spec->terminator > 255) throw std::invalid_argument("learn: terminator must be in [-1, 255]");
  const int hash_bits = checked_hash_bits("learn", spec->hash_bits);
  if (spec->reserved != 0) throw std::invalid_argument("learn: reserved must be 0");
  if (spec->n_reserved < 0 || spec->n_reserved > (1 << 20)) throw std::invalid_argument("learn: n_reserved must be in [0, 2^20]");
  if (spec->n_reserved != 0 && (!spec->reserved_tokens || !spec->reserved_off)) throw std::invalid_argument("learn: reserved_tokens or reserved_off is NULL");
  LearnPlan p;
  p.res_off.push_back(0);
  for (int64_t r = 0; r < spec->n_reserved; r++) {
    const int64_t a = spec->reserved_off[r], b = spec->reserved_off[r + 1];
    if (a < 0 || b <= a || b - a > (1 << 20)) throw std::invalid_argument("learn: reserved_tokens: token " + std::to_string(r) + " is empty or its offsets descend");
    for (int64_t k = a; k < b; k++) {
      if (spec->reserved_tokens[k] == '\n') throw std::invalid_argument("learn: reserved_tokens: token " + std::to_string(r) + " holds a line feed");
    }
    p.res.insert(p.res.end(), spec->reserved_tokens + a, spec->reserved_tokens + b);
    p.res_off.push_back(static_cast<uint32_t>(p.res.size()));
  }
  p.vocab_size = spec->vocab_size;
  p.lower = spec->lower_thresh;
  p.upper = spec->upper_thresh;
  p.slack = spec->slack;
  p.iterations = spec->num_iterations;
  p.max_chars = spec->max_token_chars;
  p.max_unique = spec->max_unique_chars;
  p.terminator = spec->terminator;
  p.hash_bits = hash_bits;
  return p;
}

// the statistics of a learn call before anything is known of its table
static wp_learn_stats &begin_learn_stats(wp_vocab *v, size_t n_words) {
  v->stats.learn_call = 1;
  v->stats.learn = wp_learn_stats{};
  v->stats.learn.n_words = static_cast<int64_t>(n_words);
  return v->stats.learn;
}

// a table in device memory
struct LearnIn {
  const uint8_t *d_pool = nullptr;
  size_t n_bytes = 0;
  const long long *d_word_off = nullptr, *d_counts = nullptr;
  size_t n_words = 0;
};

static void check_learn_sizes(size_t n_bytes, size_t n_words) {
  if (n_bytes > static_cast<size_t>(UINT32_MAX)) throw std::length_error("learn: a pool of more than UINT32_MAX bytes");
  if (n_words >= (size_t(1) << 31)) throw std::length_error("learn: the table has 2^31 words or more");
}

// the list of a table without words, the reserved tokens alone: no device needed
static wp_learned_vocab learn_reserved_only(wp_vocab *v, const LearnPlan &plan) {
  begin_learn_stats(v, 0);
  const size_t n_res = plan.res_off.size() - 1;
  wp_learned_vocab h{};
  h.n_tokens = static_cast<int64_t>(n_res);
  h.n_bytes = static_cast<int64_t>(plan.res.size() + n_res);
  h.token_off = static_cast<int64_t *>(zeroed((n_res + 1) * sizeof(int64_t)));
  if (n_res == 0) return h;
  h.scores = static_cast<int64_t *>(zeroed(n_res * sizeof(int64_t)));
  h.tokens = static_cast<uint8_t *>(zeroed(static_cast<size_t>(h.n_bytes)));
  size_t at = 0;
  for (size_t r = 0; r < n_res; r++) {
    const size_t len = plan.res_off[r + 1] - plan.res_off[r];
    std::memcpy(h.tokens + at, plan.res.data() + plan.res_off[r], len);
    h.tokens[at + len] = '\n';
    at += len + 1;
    h.token_off[r + 1] = static_cast<int64_t>(at);
  }
  return h;
}

// The list learned from the table `in`, on c's stream.  The results are device pointers into c->learn_out, valid until
// the handle's next learn call.  Waits: the table check with the characters, the sizes, one per grouping round, the
// level bounds, one per search step, the list.
static void learn_on_device(wp_vocab *v, Context *c, const LearnIn &in, const LearnPlan &plan, wp_learned_vocab *R) {
  wp_learn_stats &ls = begin_learn_stats(v, in.n_words);
  *R = wp_learned_vocab{};
  hipStream_t st = c->stream;
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  const bool timing = v->stage_timing;
  const int term = plan.terminator >= 0 ? 1 : 0;
  const size_t n = in.n_words, n1 = n + 1, n_res = plan.res_off.size() - 1, res_bytes = plan.res.size();
  RadixStats *rs = nullptr;
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkStart], st));

  // ---- the table check, the filters, the characters ---------------------------------------------------------------
  const size_t ccap = std::max<size_t>(1, std::min<size_t>(kLearnCps, in.n_bytes));  // no more characters than bytes
  const size_t ctmp_words = radix_tmp_words<uint64_t>(ccap);
  const bool rank = plan.max_unique > 0;
  Arena aux(&c->learn_aux, guard);
  uint8_t *d_res = nullptr;
  uint32_t *d_res_off = nullptr, *d_wlen = nullptr, *d_nitems = nullptr, *d_item_off = nullptr, *d_ncells = nullptr, *d_cell_off = nullptr,
           *d_present = nullptr, *d_cpos = nullptr, *d_char_cp = nullptr, *d_cv0 = nullptr, *d_cv1 = nullptr, *d_crtmp = nullptr, *d_stmp = nullptr,
           *d_bounds = nullptr;
  unsigned long long *d_occ = nullptr;
  uint64_t *d_ck0 = nullptr, *d_ck1 = nullptr;
  int32_t *d_char_group = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_res = aux.take<uint8_t>(res_bytes + 1);
    d_res_off = aux.take<uint32_t>(n_res + 1);
    d_wlen = aux.take<uint32_t>(n1);
    d_nitems = aux.take<uint32_t>(n1);
    d_item_off = aux.take<uint32_t>(n1);
    d_ncells = aux.take<uint32_t>(n1);
    d_cell_off = aux.take<uint32_t>(n1);
    d_present = aux.take<uint32_t>(kLearnCps);
    d_cpos = aux.take<uint32_t>(kLearnCps);
    d_occ = aux.take<unsigned long long>(rank ? kLearnCps : 1);
    d_char_cp = aux.take<uint32_t>(ccap);
    d_ck0 = aux.take<uint64_t>(ccap);
    d_ck1 = aux.take<uint64_t>(ccap);
    d_cv0 = aux.take<uint32_t>(ccap);
    d_cv1 = aux.take<uint32_t>(ccap);
    d_crtmp = aux.take<uint32_t>(ctmp_words);
    d_stmp = aux.take<uint32_t>(cdiv(std::max<size_t>(kLearnCps, n1), kScanTile) + 8);
    d_bounds = aux.take<uint32_t>(2 * (kLearnMaxChars + 1));
    d_char_group = aux.take<int32_t>(2 * ccap);
    if (pass == 0) aux.commit();
  }
  aux.arm(st);
  unsigned long long *d_bad = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarLearnBad);
  unsigned long long *d_counters = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarLearn);
  clear_scalars(c, kScalarLearnBad, kScalarLearn, st);
  WP_HIP(hipMemsetAsync(d_bad, 0xff, sizeof(unsigned long long), st));
  if (res_bytes) WP_HIP(hipMemcpyAsync(d_res, plan.res.data(), res_bytes, hipMemcpyHostToDevice, st));
  WP_HIP(hipMemcpyAsync(d_res_off, plan.res_off.data(), (n_res + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  // the present characters in code point order (with their weighted occurrences as rank keys where a ranking follows)
  auto list_chars = [&](bool with_occ) {
    WP_HIP(hipMemsetAsync(d_present, 0, kLearnCps * sizeof(uint32_t), st));
    if (with_occ) WP_HIP(hipMemsetAsync(d_occ, 0, kLearnCps * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(learn_chars_kernel, count_grid(n), dim3(kBlock), 0, st, in.d_pool, in.d_word_off, in.d_counts, d_wlen, n, d_present,
                       with_occ ? d_occ : static_cast<unsigned long long *>(nullptr));
    device_exclusive_scan(d_present, d_cpos, kLearnCps, d_stmp, c->d_scalars + kScalarLearnChars, st);
    hipLaunchKernelGGL(learn_char_list_kernel, count_grid(kLearnCps), dim3(kBlock), 0, st, d_present, d_cpos, d_occ, ccap, d_char_cp,
                       with_occ ? d_ck0 : static_cast<uint64_t *>(nullptr));
  };
  hipLaunchKernelGGL(learn_words_kernel, count_grid(n), dim3(kBlock), 0, st, in.d_pool, in.n_bytes, in.d_word_off, in.d_counts, n, term, d_res, d_res_off,
                     static_cast<int>(n_res), static_cast<uint32_t>(plan.max_chars), d_wlen, d_bad, d_counters);
  list_chars(rank);
  WP_LAUNCH_CHECK();
  queue_scalar_slots(c, kScalarLearnBad, kScalarLearnChars, st);
  WP_HIP(hipStreamSynchronize(st));
  unsigned long long bad;
  std::memcpy(&bad, c->h_scalars + kScalarLearnBad, sizeof(bad));
  if (bad != ~0ull) {
    const std::string w = std::to_string(bad >> 3);
    const int kind = static_cast<int>(bad & 7);
    throw std::invalid_argument(kind == kLearnBadOffsets ? "learn: word_off descends or leaves the pool at word " + w
                                : kind == kLearnBadCount ? "learn: counts: the count of word " + w + " is negative"
                                                         : "learn: words: word " + w + " is not valid UTF-8");
  }
  size_t n_chars = c->h_scalars[kScalarLearnChars];
  if (rank && n_chars > static_cast<size_t>(plan.max_unique)) {
    const int cur = radix_sort_pairs<uint64_t>(d_ck0, d_cv0, d_ck1, d_cv1, n_chars, 0, 64, d_crtmp, ctmp_words, st, rs, true);
    WP_HIP(hipMemsetAsync(d_present, 0, kLearnCps * sizeof(uint32_t), st));
    hipLaunchKernelGGL(learn_allow_kernel, count_grid(n_chars), dim3(kBlock), 0, st, cur ? d_cv1 : d_cv0, d_char_cp, n_chars,
                       static_cast<size_t>(plan.max_unique), d_present);
    hipLaunchKernelGGL(learn_char_filter_kernel, count_grid(n), dim3(kBlock), 0, st, in.d_pool, in.d_word_off, n, d_present, d_wlen, d_counters);
    list_chars(false);
  }
  // ---- the items and the cells of every remaining word ------------------------------------------------------------
  hipLaunchKernelGGL(learn_sizes_kernel, count_grid(n1), dim3(kBlock), 0, st, d_wlen, n, d_nitems, d_ncells);
  device_exclusive_scan(d_nitems, d_item_off, n1, d_stmp, nullptr, st, nullptr, reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarLearnItems));
  device_exclusive_scan(d_ncells, d_cell_off, n1, d_stmp, c->d_scalars + kScalarLearnCells, st);
  WP_LAUNCH_CHECK();
  queue_scalar_slots(c, kScalarLearnItems, kScalarLearn, st);
  WP_HIP(hipStreamSynchronize(st));
  unsigned long long items64, counters[kLearnCounters];
  std::memcpy(&items64, c->h_scalars + kScalarLearnItems, sizeof(items64));
  std::memcpy(counters, c->h_scalars + kScalarLearn, sizeof(counters));
  n_chars = c->h_scalars[kScalarLearnChars];
  ls.n_reserved = static_cast<int64_t>(counters[kLearnReserved]);
  ls.n_long = static_cast<int64_t>(counters[kLearnLong]);
  ls.n_char_dropped = static_cast<int64_t>(counters[kLearnCharDropped]);
  ls.n_chars = static_cast<int64_t>(n_chars);
  ls.n_occurrences = static_cast<int64_t>(items64);
  if (items64 >= (1ull << 31)) throw std::length_error("learn: the table has 2^31 substring occurrences or more");
  const size_t M = static_cast<size_t>(items64), n_cells = c->h_scalars[kScalarLearnCells];

  const size_t M1 = M + 1, tmp_words = radix_tmp_words<uint64_t>(M);
  Arena ia(&c->learn_items, guard);
  uint32_t *d_item_word = nullptr, *d_list0 = nullptr, *d_list1 = nullptr, *d_head = nullptr, *d_run = nullptr, *d_head_pos = nullptr, *d_left = nullptr,
           *d_left_pos = nullptr, *d_v0 = nullptr, *d_v1 = nullptr, *d_gfirst = nullptr, *d_rtmp = nullptr, *d_istmp = nullptr, *d_cell = nullptr;
  uint16_t *d_item_se = nullptr;
  int32_t *d_item_group = nullptr;
  uint64_t *d_k0 = nullptr, *d_k1 = nullptr;
  uint8_t *d_active = nullptr;
  size_t n_groups = 0;
  if (M != 0) {
    for (int pass = 0; pass < 2; pass++) {
      d_item_word = ia.take<uint32_t>(M);
      d_item_se = ia.take<uint16_t>(M);
      d_item_group = ia.take<int32_t>(M);
      d_list0 = ia.take<uint32_t>(M);
      d_list1 = ia.take<uint32_t>(M);
      d_head = ia.take<uint32_t>(M1);
      d_run = ia.take<uint32_t>(M1);
      d_head_pos = ia.take<uint32_t>(M1);
      d_left = ia.take<uint32_t>(M1);
      d_left_pos = ia.take<uint32_t>(M1);
      d_k0 = ia.take<uint64_t>(M);
      d_k1 = ia.take<uint64_t>(M);
      d_v0 = ia.take<uint32_t>(M);
      d_v1 = ia.take<uint32_t>(M);
      d_gfirst = ia.take<uint32_t>(M);
      d_rtmp = ia.take<uint32_t>(tmp_words);
      d_istmp = ia.take<uint32_t>(cdiv(M1, kScanTile) + 8);
      d_cell = ia.take<uint32_t>(n_cells);
      d_active = ia.take<uint8_t>(n_cells);
      if (pass == 0) ia.commit();
    }
    ia.arm(st);
    hipLaunchKernelGGL(learn_cells_kernel, count_grid(n), dim3(kBlock), 0, st, in.d_pool, in.d_word_off, d_wlen, d_cell_off, n, n_cells, d_cell);
    hipLaunchKernelGGL(learn_items_kernel, count_grid(M), dim3(kBlock), 0, st, d_item_off, d_wlen, n, M, d_item_word, d_item_se, d_list0);
    WP_HIP(hipMemsetAsync(d_item_group, 0xff, M * sizeof(int32_t), st));
    WP_LAUNCH_CHECK();
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));

  // ---- the rounds: hash, sort, compare with the head of the run, leftovers on ----------------------------------------
  {
    const uint64_t mask = plan.hash_bits >= 64 ? ~0ull : (1ull << plan.hash_bits) - 1ull;
    uint32_t *list = d_list0, *next = d_list1;
    size_t m = M;
    while (m != 0) {
      hipLaunchKernelGGL(learn_keys_kernel, count_grid(m), dim3(kBlock), 0, st, in.d_pool, d_item_word, d_item_se, d_cell_off, d_cell, list, m, M,
                         static_cast<uint64_t>(ls.n_rounds), mask, d_k0);
      const int cur = radix_sort_pairs<uint64_t>(d_k0, d_v0, d_k1, d_v1, m, 0, plan.hash_bits, d_rtmp, tmp_words, st, rs, true);
      const uint64_t *keys = cur ? d_k1 : d_k0;
      const uint32_t *vals = cur ? d_v1 : d_v0;
      uint32_t *d_runs = c->d_scalars + kScalarLearnRuns;
      group_runs(keys, m, d_head, d_run, d_head_pos, d_istmp, d_runs, st);
      hipLaunchKernelGGL(learn_verify_kernel, count_grid(m), dim3(kBlock), 0, st, in.d_pool, d_item_word, d_item_se, d_cell_off, d_cell, list, vals, d_head,
                         d_run, d_head_pos, m, M, static_cast<uint32_t>(n_groups), d_left, d_item_group);
      hipLaunchKernelGGL(learn_group_first_kernel, count_grid(m), dim3(kBlock), 0, st, list, vals, d_head_pos, d_runs, m, d_gfirst + n_groups);
      carry_leftovers(d_left, d_left_pos, m, list, next, d_istmp, c->d_scalars + kScalarLearnLeft, st);
      n_groups += end_round(c, kScalarLearnRuns, kScalarLearnLeft, "learn", "occurrence", &m, &ls, st);
      std::swap(list, next);
    }
  }
  ls.n_tokens = static_cast<int64_t>(n_groups);
  const size_t G = n_groups;

  // ---- per token: parent, level order; the items in the order of their groups; the groups of the characters ----------
  Arena ga(&c->learn_groups, guard);
  int32_t *d_parent = nullptr;
  unsigned long long *d_sum = nullptr;
  uint32_t *d_kept = nullptr, *d_level = nullptr, *d_flag = nullptr, *d_fpos = nullptr, *d_listed = nullptr;
  std::array<uint32_t, 2 * (kLearnMaxChars + 1)> bounds{};
  const uint32_t *d_perm = nullptr;
  const uint64_t *d_gkey = nullptr;
  if (G != 0) {
    for (int pass = 0; pass < 2; pass++) {
      d_parent = ga.take<int32_t>(G);
      d_sum = ga.take<unsigned long long>(G);
      d_kept = ga.take<uint32_t>(G);
      d_level = ga.take<uint32_t>(G);
      d_flag = ga.take<uint32_t>(G + 1);
      d_fpos = ga.take<uint32_t>(G + 1);
      d_listed = ga.take<uint32_t>(G);
      if (pass == 0) ga.commit();
    }
    ga.arm(st);
    hipLaunchKernelGGL(learn_group_info_kernel, count_grid(G), dim3(kBlock), 0, st, d_gfirst, d_item_se, d_item_group, G, M, d_k0, d_parent);
    int cur = radix_sort_pairs<uint64_t>(d_k0, d_v0, d_k1, d_v1, G, 0, 7, d_rtmp, tmp_words, st, rs, true);
    WP_HIP(hipMemcpyAsync(d_level, cur ? d_v1 : d_v0, G * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    WP_HIP(hipMemsetAsync(d_bounds, 0, bounds.size() * sizeof(uint32_t), st));
    hipLaunchKernelGGL(learn_level_bounds_kernel, count_grid(G), dim3(kBlock), 0, st, cur ? d_k1 : d_k0, G, d_bounds);
    WP_HIP(hipMemcpyAsync(bounds.data(), d_bounds, bounds.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    WP_HIP(hipStreamSynchronize(st));  // (the sort below takes the key buffers over)
    hipLaunchKernelGGL(learn_group_keys_kernel, count_grid(M), dim3(kBlock), 0, st, d_item_group, M, d_k0);
    cur = radix_sort_pairs<uint64_t>(d_k0, d_v0, d_k1, d_v1, M, 0, std::max(1, bit_length(G)), d_rtmp, tmp_words, st, rs, true);
    d_perm = cur ? d_v1 : d_v0;
    d_gkey = cur ? d_k1 : d_k0;
    WP_HIP(hipMemsetAsync(d_char_group, 0xff, 2 * ccap * sizeof(int32_t), st));
    const size_t n_single = bounds[kLearnMaxChars + 1 + 1] - bounds[1];
    hipLaunchKernelGGL(learn_char_groups_kernel, count_grid(n_single), dim3(kBlock), 0, st, in.d_pool, d_level + bounds[1], n_single, d_gfirst, d_item_word,
                       d_item_se, d_cell_off, d_cell, d_char_cp, n_chars, G, M, d_char_group);
    WP_LAUNCH_CHECK();
  }
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));

  // ---- the search ----------------------------------------------------------------------------------------------------
  size_t n_listed = 0;
  long long thresh = 0;
  if (G != 0) {
    long long lower = plan.lower, upper = plan.upper;
    for (;;) {
      const long long t = lower + (upper - lower) / 2;  // ((lower + upper) / 2 without the overflow; both are positive)
      ls.n_steps++;
      for (int it = 0; it < plan.iterations; it++) {
        if (it != 0) {
          hipLaunchKernelGGL(learn_split_kernel, count_grid(n), dim3(kBlock), 0, st, d_wlen, d_item_off, d_cell_off, d_item_group, d_kept, n, M, G, n_cells,
                             d_active);
        }
        WP_HIP(hipMemsetAsync(d_sum, 0, G * sizeof(unsigned long long), st));
        hipLaunchKernelGGL(learn_sum_kernel, count_grid(M), dim3(kBlock), 0, st, d_perm, d_gkey, d_item_word, d_item_se, d_cell_off, in.d_counts,
                           it != 0 ? d_active : static_cast<const uint8_t *>(nullptr), M, G, d_sum);
        clear_scalars(c, kScalarLearnKept, kScalarLearnKept, st);
        for (int len = plan.max_chars; len >= 1; len--) {  // (the level order is the launch order)
          const size_t lo = bounds[len], cnt = bounds[kLearnMaxChars + 1 + len] - lo;
          if (cnt == 0) continue;
          hipLaunchKernelGGL(learn_level_kernel, count_grid(cnt), dim3(kBlock), 0, st, d_level + lo, cnt, t, G, d_parent, d_sum, d_kept,
                             len >= 2 ? c->d_scalars + kScalarLearnKept : static_cast<uint32_t *>(nullptr));
        }
      }
      WP_LAUNCH_CHECK();
      queue_scalar_slots(c, kScalarLearnKept, kScalarLearnKept, st);
      WP_HIP(hipStreamSynchronize(st));
      n_listed = c->h_scalars[kScalarLearnKept];
      const long long size = static_cast<long long>(n_res + 2 * n_chars + n_listed);
      thresh = t;
      if ((size <= plan.vocab_size && plan.vocab_size - size <= plan.slack) || lower >= upper || t <= 1) break;
      if (size > plan.vocab_size) lower = t + 1; else upper = t - 1;
    }
  }
  ls.thresh = thresh;
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkScanned], st));

  // ---- the list: order, entries, offsets, text -----------------------------------------------------------------------
  const size_t E = n_res + 2 * n_chars + n_listed;
  // (no wait for the bytes of the text before its room is taken: no entry is longer than "##", 64 characters and '\n')
  const size_t text_cap = res_bytes + n_res + 2 * n_chars * 7 + n_listed * (4 * kLearnMaxChars + 3);
  Arena oa(&c->learn_out, guard);
  uint8_t *d_text = nullptr, *d_from = nullptr;
  long long *d_token_off = nullptr, *d_scores = nullptr;
  uint32_t *d_len = nullptr, *d_len_pos = nullptr, *d_src = nullptr, *d_ostmp = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    d_text = oa.take<uint8_t>(text_cap);
    d_token_off = oa.take<long long>(E + 1);
    d_scores = oa.take<long long>(E);
    d_len = oa.take<uint32_t>(E + 1);
    d_len_pos = oa.take<uint32_t>(E + 1);
    d_src = oa.take<uint32_t>(E);
    d_from = oa.take<uint8_t>(E);
    d_ostmp = oa.take<uint32_t>(cdiv(E + 1, kScanTile) + 8);
    if (pass == 0) oa.commit();
  }
  oa.arm(st);
  const uint32_t *d_ordered = nullptr;
  if (n_listed != 0) {  // (the search is over: the sort buffers are free again)
    hipLaunchKernelGGL(learn_listed_kernel, count_grid(G), dim3(kBlock), 0, st, d_kept, d_parent, G, d_flag);
    device_exclusive_scan(d_flag, d_fpos, G, d_istmp, nullptr, st);
    hipLaunchKernelGGL(learn_first_keys_kernel, count_grid(G), dim3(kBlock), 0, st, d_flag, d_fpos, d_gfirst, G, n_listed, d_k0, d_listed);
    const int a = radix_sort_pairs<uint64_t>(d_k0, d_v0, d_k1, d_v1, n_listed, 0, std::max(1, bit_length(M)), d_rtmp, tmp_words, st, rs, true);
    uint64_t *ka = a ? d_k1 : d_k0, *kb = a ? d_k0 : d_k1;  // a: the pair that holds the order by first item; b: the other
    uint32_t *va = a ? d_v1 : d_v0, *vb = a ? d_v0 : d_v1;
    hipLaunchKernelGGL(learn_score_keys_kernel, count_grid(n_listed), dim3(kBlock), 0, st, va, d_listed, d_sum, n_listed, G, kb, vb);
    const int b = radix_sort_pairs<uint64_t>(kb, vb, ka, va, n_listed, 0, 64, d_rtmp, tmp_words, st, rs, false);  // (stable: ties keep the first order)
    d_ordered = b ? va : vb;
  }
  hipLaunchKernelGGL(learn_emit_kernel, count_grid(E + 1), dim3(kBlock), 0, st, d_res_off, n_res, d_char_cp, d_char_group, n_chars, d_ordered, n_listed,
                     d_gfirst, d_item_word, d_item_se, d_cell_off, d_cell, d_kept, d_sum, G, M, d_scores, d_len, d_src, d_from);
  device_exclusive_scan(d_len, d_len_pos, E + 1, d_ostmp, c->d_scalars + kScalarLearnOutBytes, st);
  hipLaunchKernelGGL(group_offsets_kernel, count_grid(E + 1), dim3(kBlock), 0, st, d_len_pos, E, 0, d_token_off);
  hipLaunchKernelGGL(learn_gather_kernel, count_grid(text_cap), dim3(kBlock), 0, st, in.d_pool, in.n_bytes, d_res, res_bytes, d_token_off, d_src, d_from, E,
                     text_cap, d_text);
  WP_LAUNCH_CHECK();
  queue_scalar_slots(c, kScalarLearnOutBytes, kScalarLearnOutBytes, st);
  if (timing) WP_HIP(hipEventRecord(c->ev[kMarkWalked], st));
  WP_HIP(hipStreamSynchronize(st));
  const size_t out_bytes = c->h_scalars[kScalarLearnOutBytes];
  if (out_bytes > text_cap) throw HipError("learn: the list is longer than its bound");
  if (timing) {  // wp_stats, as the header's section says: the stage times of this call in the fields an encode times itself in
    const float table = mark_ms(c, kMarkStart, kMarkCounted), groups = mark_ms(c, kMarkCounted, kMarkSorted), search = mark_ms(c, kMarkSorted, kMarkScanned),
                list = mark_ms(c, kMarkScanned, kMarkWalked);
    v->stats.ms_decode = table;
    v->stats.ms_sa = groups;
    v->stats.ms_scan = search;
    v->stats.ms_walk = list;
    v->stats.ms_total = table + groups + search + list;
  }
  throw_if_group_oob(kSiteLearn, "vocabulary learner", "stores or gathers outside the item, group or list arrays skipped");
  check_arena_guard(c, aux, st, "learn");
  check_arena_guard(c, ia, st, "learn");
  check_arena_guard(c, ga, st, "learn");
  check_arena_guard(c, oa, st, "learn");
  R->tokens = out_bytes ? d_text : nullptr;
  R->token_off = reinterpret_cast<int64_t *>(d_token_off);
  R->scores = E ? reinterpret_cast<int64_t *>(d_scores) : nullptr;
  R->n_tokens = static_cast<int64_t>(E);
  R->n_bytes = static_cast<int64_t>(out_bytes);
  R->thresh = thresh;
}

}  // namespace wp
