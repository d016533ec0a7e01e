// repetition_path.h — the repetition signals on a context (include/wordpiece_amd_repetition.h; kernels: repetition.h):
// the argument rules, the answer of a call without bytes, the launches over one device batch and the buffers of a call.
// The intake, the class pass with the word list, the word identities and the end of a call are text_path.h's.
#pragma once
#include <algorithm>

#include "context.h"
#include "repetition.h"
#include "text_path.h"

namespace wp {

struct RepetitionPlan {
  bool want_compact = false;
  RptLimits lim{};
};

// every rule of the spec, each with the field it is about; nothing here needs a device
static RepetitionPlan check_repetition_spec(const wp_repetition_spec *spec, const wp_repetition_result *out) {
  if (!spec) throw std::invalid_argument("repetition: spec is NULL");
  if (!out) throw std::invalid_argument("repetition: out is NULL");
  if (spec->elem_bytes != 1) throw std::invalid_argument("repetition: elem_bytes must be 1");
  check_want("repetition", spec->want, WP_RPT_WANT_COMPACT);
  RepetitionPlan p;
  p.want_compact = (spec->want & WP_RPT_WANT_COMPACT) != 0;
  for (int k = 0; k < WP_RPT_RULES; k++) {
    const int64_t L = spec->limit[k];
    if (L < -1 || L > 1000) throw std::invalid_argument("repetition: limit[" + std::to_string(k) + "] must be -1 or in [0, 1000]");
    p.lim.v[k] = L;
  }
  if (spec->reserved != 0) throw std::invalid_argument("repetition: reserved must be 0");
  return p;
}

static_assert(kRptCounters <= kTextMaxCounters, "the counters of a text-signal layer");
constexpr TextLayer kRptLayer{"repetition", "repetition signals", "gathers or stores outside the tile, word, slot or signal arrays skipped",
                              kScalarRptBad, kScalarRptKept, kScalarRptElems, kScalarRptWindows, kScalarRptWords, kScalarRptLines, kScalarRptOutBytes,
                              kScalarRpt, kRptCounters};

static wp_repetition_stats &begin_repetition_stats(wp_vocab *v, size_t n_rows) {
  v->stats.repetition_call = 1;
  v->stats.repetition = wp_repetition_stats{};
  v->stats.repetition.n_rows = static_cast<int64_t>(n_rows);
  return v->stats.repetition;
}

// a host call whose batch has no byte (n_rows >= 1): the rules over zeros (text_path.h)
static wp_repetition_result repetition_no_bytes(wp_vocab *v, const RepetitionPlan &plan, size_t n_rows) {
  const long long zeros[WP_RPT_SIGNALS] = {};
  return text_no_bytes<wp_repetition_result>(begin_repetition_stats(v, n_rows), n_rows, WP_RPT_SIGNALS, WP_RPT_RULES, repetition_reasons(zeros, plan.lim),
                                             plan.want_compact);
}

// The batch `in` (n_rows >= 1), on c's stream.  The results are device pointers into c->repetition_rows (signals,
// reasons) and c->repetition_out (the compact form), valid until the handle's next call.  Waits: the sizes, the numbers
// of words and lines, those of the duplicate-row search over the words, with the compact form the kept count, and the
// one that ends the call.
static void repetition_on_device(wp_vocab *v, Context *c, const RaggedIn &in, const RepetitionPlan &plan, wp_repetition_result *R) {
  const TextLayer &L = kRptLayer;
  const size_t n = in.n_rows;
  wp_repetition_stats &ps = begin_repetition_stats(v, n);
  *R = wp_repetition_result{};
  R->n_rows = static_cast<int64_t>(n);
  hipStream_t st = c->stream;
  const bool guard = v->arena_guard || EnvOptions::get().arena_guard;
  // WP_OPT_STAGE_TIMING: kMarkStart, kMarkCounted (intake, class passes, word list, word identity), kMarkSorted (the
  // five sorts), kMarkScanned (the LCP and the run passes), kMarkWalked (cover, rules, compact form)
  const bool timing = v->stage_timing;
  RadixStats *rs = begin_stage_timing(c, timing, st);

  // ---- the per-row arrays, the offset check --------------------------------------------------------------------------------
  Arena ra(&c->repetition_rows, guard);
  TextRows rows;
  unsigned long long *d_top = nullptr, *d_qsig = nullptr;
  for (int pass = 0; pass < 2; pass++) {
    rows.take(ra, n, WP_RPT_SIGNALS);
    d_top = ra.take<unsigned long long>(n * kRptGroup);
    d_qsig = ra.take<unsigned long long>(n * WP_QUALITY_SIGNALS);  // what the class pass sums beside its counts: not read
    if (pass == 0) ra.commit();
  }
  ra.arm(st);
  unsigned long long *d_counters = reinterpret_cast<unsigned long long *>(c->d_scalars + kScalarRpt);
  unsigned long long *d_usig = rows.usig();
  WP_HIP(hipMemsetAsync(d_top, 0, n * kRptGroup * sizeof(unsigned long long), st));
  WP_HIP(hipMemsetAsync(d_qsig, 0, n * WP_QUALITY_SIGNALS * sizeof(unsigned long long), st));
  rows.queue(c, L, in, st);
  const size_t nb = rows.read(c, L, in, st);
  ps.n_bytes = static_cast<int64_t>(nb);

  // ---- the class pass of quality.h: the numbers of words and lines -------------------------------------------------------------
  Arena ia(&c->repetition_items, guard);
  ClassPass cls;
  for (int pass = 0; pass < 2; pass++) {
    cls.take(ia, nb);
    if (pass == 0) ia.commit();
  }
  ia.arm(st);
  const ClassPass::Counts counts = cls.count(c, L, in, rows, d_qsig, st);
  const size_t nw = counts.n_words, nl = counts.n_lines;
  if (nw >= (size_t(1) << 30)) throw std::length_error("repetition: 2^30 words or more");

  // ---- the per-word arrays ---------------------------------------------------------------------------------------------------
  const size_t nw1 = nw + 1, dup_rows = 2 * nw + 1, tmp_words = radix_tmp_words<uint64_t>(nw);
  Arena la(&c->repetition_lists, guard);
  QualLists lists{};
  uint32_t *d_wchars = nullptr, *d_v0 = nullptr, *d_v1 = nullptr, *d_r1 = nullptr, *d_r2 = nullptr, *d_r4 = nullptr, *d_r8 = nullptr, *d_rtmp = nullptr,
           *d_wtmp = nullptr;
  uint64_t *d_k0 = nullptr, *d_k1 = nullptr;
  uint8_t *d_lcp = nullptr, *d_flags = nullptr;
  long long *d_dup_off = nullptr;
  RptRuns runs{};
  for (int pass = 0; pass < 2; pass++) {
    lists = ClassPass::take_lists(la, nw, nl, true);
    d_wchars = la.take<uint32_t>(nw);
    d_dup_off = la.take<long long>(dup_rows + 1);
    d_k0 = la.take<uint64_t>(nw);
    d_k1 = la.take<uint64_t>(nw);
    d_v0 = la.take<uint32_t>(nw);
    d_v1 = la.take<uint32_t>(nw);
    d_r1 = la.take<uint32_t>(nw);
    d_r2 = la.take<uint32_t>(nw);
    d_r4 = la.take<uint32_t>(nw);
    d_r8 = la.take<uint32_t>(nw);
    d_lcp = la.take<uint8_t>(nw);
    d_flags = la.take<uint8_t>(2 * nw);  // (one byte per word and run pass of n >= 5)
    for (int j = 0; j < kRptGroup; j++) {
      runs.head[j] = la.take<uint32_t>(nw1);
      runs.run[j] = la.take<uint32_t>(nw1);
      runs.aux[j] = la.take<uint32_t>(nw1);
    }
    d_rtmp = la.take<uint32_t>(tmp_words);
    d_wtmp = la.take<uint32_t>(cdiv(nw1, kScanTile) + 8);
    if (pass == 0) la.commit();
  }
  la.arm(st);
  if (nw != 0) {
    // ---- the word list, every word's characters, the word batch; the word identities ------------------------------------------
    cls.write(c, in, rows, d_qsig, lists, st);
    hipLaunchKernelGGL(rpt_word_rows_kernel, count_grid(nw), dim3(kBlock), 0, st, lists, nb, d_wchars, d_dup_off);
    WP_LAUNCH_CHECK();
    const int32_t *first = first_equal_items(v, c, in, d_dup_off, nw);
    if (timing) WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));

    // ---- r1, then the rounds: one order of the positions by their 10-word windows -------------------------------------------
    const int id_bits = bit_length(dup_rows), row_bits = std::max(1, bit_length(n - 1)), bits = bit_length(nw);
    const uint32_t *vals = nullptr;
    auto sort_and_rank = [&](int key_bits, uint32_t *rank) {
      const int cur = radix_sort_pairs<uint64_t>(d_k0, d_v0, d_k1, d_v1, nw, 0, key_bits, d_rtmp, tmp_words, st, rs, true);
      vals = cur ? d_v1 : d_v0;
      if (!rank) return;
      hipLaunchKernelGGL(group_heads_kernel, count_grid(nw), dim3(kBlock), 0, st, static_cast<const uint64_t *>(cur ? d_k1 : d_k0), nw, runs.head[0]);
      device_exclusive_scan(runs.head[0], runs.run[0], nw, d_wtmp, nullptr, st);
      hipLaunchKernelGGL(rpt_rank_kernel, count_grid(nw), dim3(kBlock), 0, st, vals, static_cast<const uint32_t *>(runs.head[0]),
                         static_cast<const uint32_t *>(runs.run[0]), nw, rank);
    };
    auto pair_keys = [&](const uint32_t *a, const uint32_t *b, uint32_t h) {
      hipLaunchKernelGGL(rpt_pair_keys_kernel, count_grid(nw), dim3(kBlock), 0, st, a, b, static_cast<const uint32_t *>(lists.wrow), nw, h, bits, d_k0);
    };
    hipLaunchKernelGGL(rpt_word_keys_kernel, count_grid(nw), dim3(kBlock), 0, st, static_cast<const uint32_t *>(lists.wrow), first, nw, id_bits, d_k0);
    sort_and_rank(id_bits + row_bits, d_r1);
    pair_keys(d_r1, d_r1, 1);
    sort_and_rank(2 * bits, d_r2);
    pair_keys(d_r2, d_r2, 2);
    sort_and_rank(2 * bits, d_r4);
    pair_keys(d_r4, d_r4, 4);
    sort_and_rank(2 * bits, d_r8);
    pair_keys(d_r8, d_r2, 8);
    sort_and_rank(2 * bits, nullptr);
    WP_LAUNCH_CHECK();
    if (timing) WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));

    // ---- the LCP of neighbours, the runs of every length three lengths at a time ----------------------------------------------
    hipLaunchKernelGGL(rpt_lcp_kernel, count_grid(nw), dim3(kBlock), 0, st, vals, static_cast<const uint32_t *>(d_r1), static_cast<const uint32_t *>(lists.wrow), nw,
                       d_lcp);
    for (uint32_t n0 = 2; n0 <= 8; n0 += kRptGroup) {
      hipLaunchKernelGGL(rpt_heads_kernel, count_grid(nw1), dim3(kBlock), 0, st, static_cast<const uint8_t *>(d_lcp), nw, n0, runs);
      for (int j = 0; j < kRptGroup; j++) device_exclusive_scan(runs.head[j], runs.run[j], nw1, d_wtmp, nullptr, st);
      if (n0 == 2) {
        hipLaunchKernelGGL(rpt_head_pos_kernel, count_grid(nw1), dim3(kBlock), 0, st, nw, runs);
        hipLaunchKernelGGL(rpt_top_kernel, count_grid(nw), dim3(kBlock), 0, st, vals, nw, runs, static_cast<const uint32_t *>(lists.wrow),
                           static_cast<const uint32_t *>(d_wchars), n, d_top);
      } else {
        for (int j = 0; j < kRptGroup; j++) WP_HIP(hipMemsetAsync(runs.aux[j], 0xff, nw1 * sizeof(uint32_t), st));
        hipLaunchKernelGGL(rpt_first_kernel, count_grid(nw), dim3(kBlock), 0, st, vals, nw, runs);
        hipLaunchKernelGGL(rpt_mark_kernel, count_grid(nw), dim3(kBlock), 0, st, vals, nw, runs, d_flags + (n0 == 5 ? 0 : nw));
      }
    }
    WP_LAUNCH_CHECK();
    if (timing) WP_HIP(hipEventRecord(c->ev[kMarkScanned], st));
    hipLaunchKernelGGL(rpt_cover_kernel, count_grid(nw), dim3(kBlock), 0, st, static_cast<const uint8_t *>(d_flags), static_cast<const uint32_t *>(lists.wrow),
                       static_cast<const uint32_t *>(d_wchars), nw, n, d_usig);
  } else if (timing) {  // (no word: the three stages in front of the rules are empty)
    WP_HIP(hipEventRecord(c->ev[kMarkCounted], st));
    WP_HIP(hipEventRecord(c->ev[kMarkSorted], st));
    WP_HIP(hipEventRecord(c->ev[kMarkScanned], st));
  }

  // ---- the rules, the kept rows, the compact form -----------------------------------------------------------------------------
  hipLaunchKernelGGL(rpt_rules_kernel, count_grid(n + 1), dim3(kBlock), 0, st, n, plan.lim, static_cast<const unsigned long long *>(d_top), rows.d_sig, rows.d_reasons,
                     rows.d_keep, d_counters);
  WP_LAUNCH_CHECK();
  Arena oa(&c->repetition_out, guard);
  TextTail tail;
  tail.begin(c, L, rows, nb, plan.want_compact, oa, st);
  // (stage timing: words, sorts, runs, cover and rules: the header's section)
  tail.end(v, c, L, rows, in, rows.d_boff, nb, plan.want_compact, {&ra, &ia, &la, &oa}, R, [&](const unsigned long long *counters, int64_t n_kept) {
    ps.n_words = static_cast<int64_t>(counters[kRptWordsTotal]);
    ps.n_word_chars = static_cast<int64_t>(counters[kRptWordChars]);
    ps.n_kept = n_kept;
    for (int k = 0; k < WP_RPT_RULES; k++) ps.rule_failed[k] = static_cast<int64_t>(counters[kRptRuleFailed + k]);
    if (static_cast<size_t>(ps.n_words) != nw) throw HipError("repetition: the rows do not sum to the words of the text");
  });
}

}  // namespace wp
